"""`from evaluation import evaluate_deer_model` (run_multimodal_deer.py:79; src/evaluation/evaluation.py:785-808).

`evaluate_deer_model` stays the trainer's (the validation dictionary the script prints).  The evaluator classes of
src/training/evaluation.py are mmdeer.evaluation's; its `evaluate_deer_model`, which returns an `EvaluationResults`, is
reachable as `DEERModelEvaluator(...).evaluate_model` or `mmdeer.evaluation.evaluate_deer_model`."""
from mmdeer.trainer import evaluate_deer_model, evaluate_loaders  # noqa: F401
from mmdeer.evaluation import (  # noqa: F401
    CalibrationAnalyzer,
    DEERModelEvaluator,
    EvaluationResults,
    StatisticalValidator,
    UncertaintyAnalyzer,
)
