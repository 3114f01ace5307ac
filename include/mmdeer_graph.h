/* mmdeer -- C ABI of what lets a training step that runs through autograd be replayed as ONE HIP graph (mmdeer/train_graph.py):
 * device-resident step counters for the BERT trunk's five dropout entries (csrc/bert_drop.hip) and for the optimiser step over any
 * list of tensors (csrc/optim_multi.hip).  A replay repeats the kernel arguments of the capture, so what must differ between steps
 * is read from device memory when the kernel runs.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the
 * ctypes binding), exported by the same library and covered by the same MMDEER_ABI_VERSION.  The argument structs of
 * include/mmdeer_bert_drop.h and the tensor record of include/mmdeer_optim.h are passed by reference and named here as opaque types.
 *
 * THE DROPOUT COUNTER.  Each entry of mmdeer_bert_drop.h has a twin mmdeer_<entry>_dev(args, offset_dev) whose second argument
 * points at ONE uint64_t in device memory, 8-byte aligned (anything else is refused).  As in mmdeer.h the effective step is
 * offset + *offset_dev (modulo 2^64), read on the device when the kernel runs: a captured graph that bumps the counter between replays
 * draws fresh masks from unchanged kernel arguments.  The host never dereferences the pointer and no launch writes the counter --
 * neither of attn_drop_bwd's two launches nor drop_add_ln_bwd's pair -- so every launch of a step sees the same value as long as the
 * caller advances it between steps only.  offset_dev == NULL IS the plain entry: one kernel text per operator, in which every wave
 * forms key(seed, offset + *offset_dev, site) once, in scalar registers from a scalar load, before its first element
 * (csrc/common.h: drop_key).  Conventions and refusals are the plain entries'; with dropout_p == 0 the plain non-dropout kernel runs
 * and the counter is not read.
 *
 * THE CAPTURABLE OPTIMISER STEP, mmdeer_adamw_multi_dev: mmdeer_adamw_multi's step (include/mmdeer_optim.h: the same tensor records,
 * table, moments, scratch, launches and arithmetic) for a stream capture.  What a replay must see change lives in device memory the
 * caller owns: `classes`, nclasses records of mmdeer_adamw_multi_class_dev, 16-byte aligned, whose `step` counts the steps DONE so
 * far.  Workgroup 0 of launch 1 adds 1 to every listed class's step; launch 2 reads the new value across the kernel boundary, so none
 * of its workgroups races the increment, and forms bc = 1 - beta^step once per workgroup (never per element): beta^step by repeated
 * squaring in float64, rounded once to float32 -- not the host's powf, so the two entries may differ in the last bit of a bias
 * correction.  lr and weight_decay are read from the record; the caller rewrites them with an ordinary copy when they change.  Still
 * two launches and no atomics; a call with no element to update launches nothing and advances no step.
 *   upload != 0 writes the table with launches alone: the records ride in the kernel arguments of a table-writing kernel, a batch
 * that fits 4 KiB per launch, and one more kernel derives the chunk -> tensor map from them on the device.  No copy, no second
 * stream, no wait: the call reads no host memory after it returns, and a capture records the upload with the step as one linear
 * chain.  mmdeer_adamw_multi_dev_uploads counts these; mmdeer_adamw_multi_blocking_calls counts the waits for a stream that
 * mmdeer_adamw_multi's uploads have made -- neither it nor mmdeer_adamw_multi_uploads moves inside a capture.
 *   Refusals are mmdeer_adamw_multi's without the classes' own (device data: the caller validates lr and weight_decay), plus a NULL
 * or misaligned `classes`. */
#ifndef MMDEER_GRAPH_H_
#define MMDEER_GRAPH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmdeer_bert_embed_drop_args mmdeer_bert_embed_drop_args;
typedef struct mmdeer_bert_attn_drop_args mmdeer_bert_attn_drop_args;
typedef struct mmdeer_bert_drop_add_ln_args mmdeer_bert_drop_add_ln_args;
typedef struct mmdeer_bert_attn_drop_bwd_args mmdeer_bert_attn_drop_bwd_args;
typedef struct mmdeer_bert_drop_add_ln_bwd_args mmdeer_bert_drop_add_ln_bwd_args;
typedef struct mmdeer_adamw_multi_tensor mmdeer_adamw_multi_tensor;

int mmdeer_bert_embed_drop_fwd_dev(const mmdeer_bert_embed_drop_args* a, const uint64_t* offset_dev);
int mmdeer_bert_attn_drop_fwd_dev(const mmdeer_bert_attn_drop_args* a, const uint64_t* offset_dev);
int mmdeer_bert_drop_add_ln_fwd_dev(const mmdeer_bert_drop_add_ln_args* a, const uint64_t* offset_dev);
int mmdeer_bert_attn_drop_bwd_dev(const mmdeer_bert_attn_drop_bwd_args* a, const uint64_t* offset_dev);
int mmdeer_bert_drop_add_ln_bwd_dev(const mmdeer_bert_drop_add_ln_bwd_args* a, const uint64_t* offset_dev);

typedef struct mmdeer_adamw_multi_class_dev {
  float lr, weight_decay;
  int32_t step;             /* steps DONE so far: the call adds 1 on the device, then uses the sum */
  int32_t reserved;
} mmdeer_adamw_multi_class_dev;

typedef struct mmdeer_adamw_multi_dev_args {
  const mmdeer_adamw_multi_tensor* tensors;       /* host records, as for mmdeer_adamw_multi */
  int32_t ntensors, nclasses;
  void* classes;                                  /* device memory: nclasses mmdeer_adamw_multi_class_dev, 16-byte aligned */
  float* exp_avg; float* exp_avg_sq;
  long long moment_elems;
  void* table;
  long long table_bytes;
  int32_t upload;                                 /* nonzero: write the table from the records, by launches on `stream` */
  int32_t reserved;
  float* scratch;
  float* grad_norm;
  float beta1, beta2, eps, max_grad_norm, grad_scale;
  void* stream;
} mmdeer_adamw_multi_dev_args;
int mmdeer_adamw_multi_dev(const mmdeer_adamw_multi_dev_args* a);
/* how many table uploads mmdeer_adamw_multi_dev has made in this process */
long long mmdeer_adamw_multi_dev_uploads(void);
/* how many times mmdeer_adamw_multi has waited for a stream in this process */
long long mmdeer_adamw_multi_blocking_calls(void);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_GRAPH_H_ */
