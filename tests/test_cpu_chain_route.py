"""The kernel a layer-chain launch runs (csrc/chain.hip: chain_route), asked of the library's dry runs (include/mmdeer_routes.h) --
no GPU is touched: mmdeer_chain_route for one mmdeer_chain call, mmdeer_step_chain_routes for the chain launches of a Stack C
training step.  16-sample workgroups run the 4-deep kernel (s16), option chain_depth = 2 / 8 its A/B instantiations, 32-sample
workgroups (a batch above 4096, or forced) s32."""
import ctypes as C

import pytest

from mmdeer import _lib

A = 1 << 20          # a plausible, aligned address: the dry run dereferences none


def chain_route(rows, ts=0, **edit):
    """(return code, text) of mmdeer_chain_route on a one-layer 256 -> 256 table."""
    a = _lib.ChainArgs()
    a.X, a.ldx, a.K0, a.rows, a.samples_per_workgroup, a.nseg = A, 256, 256, rows, ts, 1
    s = a.seg[0]
    s.W, s.N, s.K, s.end_layer, s.nout, s.drop_site, s.mask_scale = A, 256, 256, 1, 256, -1, 1.0
    for k, v in edit.items():
        setattr(s, k, v)
    out = C.create_string_buffer(64)
    rc = _lib.load().mmdeer_chain_route(C.byref(a), out, len(out))
    return rc, out.value.decode()


def step_routes(B, targets=1, inputs_bf16=1, f32=0):
    out = C.create_string_buffer(256)
    n = _lib.load().mmdeer_step_chain_routes(B, f32, inputs_bf16, targets, out, len(out))
    lines = [ln.split(" ") for ln in out.value.decode().split("\n") if ln]
    assert n == len(lines)
    return dict(lines)


def test_default_options_give_the_four_deep_kernel():
    assert _lib.get_option("chain_depth") == 4
    for rows in (1, 16, 17, 4096):
        assert chain_route(rows) == (1, f"s16 workgroups={(rows + 15) // 16}")
    assert chain_route(8192, ts=16) == (1, "s16 workgroups=512")
    for B in (512, 4096):
        assert step_routes(B) == {"F1-F6": "s16", "F9-F17": "s16", "B1-B10": "s16", "B13-B17": "s16"}
    # fp32 feature blocks: no input chain, the audio-visual chain starts at F2
    assert list(step_routes(4096, inputs_bf16=0)) == ["F2-F6", "F9-F17", "B1-B10", "B13-B17"]


@pytest.mark.parametrize("depth,kernel", [(2, "s16_d2"), (8, "s16_d8"), (6, "s16")])
def test_chain_depth_selects_the_16_sample_instantiation(depth, kernel):
    with _lib.options(chain_depth=depth):
        assert chain_route(40) == (1, f"{kernel} workgroups=3")
        assert set(step_routes(4096).values()) == {kernel}
        assert chain_route(4097) == (1, "s32 workgroups=129")          # the 32-sample kernel has one depth
    assert chain_route(40) == (1, "s16 workgroups=3")                  # restored


def test_a_batch_above_4096_gives_the_32_sample_kernel():
    assert chain_route(4097) == (1, "s32 workgroups=129")
    assert chain_route(40, ts=32) == (1, "s32 workgroups=2")
    assert set(step_routes(8192).values()) == {"s32"}
    with _lib.options(chain_ts=32):
        assert chain_route(40) == (1, "s32 workgroups=2")
        assert set(step_routes(4096).values()) == {"s32"}


def test_the_step_query_follows_the_plan():
    assert step_routes(256) == {}                                   # below chain_min: launch by launch
    assert step_routes(4096, f32=1) == {}
    assert step_routes(0) == {}
    with _lib.options(chain_bwd=0):
        assert list(step_routes(4096)) == ["F1-F6", "F9-F17"]
    with _lib.options(chain_nig=0):                                  # the head's backward as a launch of its own
        assert list(step_routes(4096)) == ["F1-F6", "F9-F17", "B2-B10", "B13-B17"]
    assert list(step_routes(4096, targets=0)) == ["F1-F6", "F9-F17", "B2-B10", "B13-B17"]
    with _lib.options(chain_nigf=1):                                 # the NIG head as the forward chain's tail
        assert list(step_routes(4096)) == ["F1-F6", "F9-F18", "B1-B10", "B13-B17"]
    lib = _lib.load()
    assert lib.mmdeer_step_chain_routes(4096, 0, 1, 1, None, 0) == 4                     # the count alone
    out = C.create_string_buffer(9)
    assert lib.mmdeer_step_chain_routes(4096, 0, 1, 1, out, len(out)) == 4 and out.value == b"F1-F6 s1"   # truncated, NUL-terminated
    assert lib.mmdeer_step_chain_routes(-1, 0, 1, 1, None, 0) == -1


def test_the_dry_run_refuses_what_the_call_refuses():
    lib = _lib.load()
    assert chain_route(0) == (0, "")                                # an empty batch is nothing to do
    rc, _ = chain_route(40, K=320)
    assert rc == -1 and b"chain" in lib.mmdeer_last_error()         # K = 320 reads past the 256-wide input panel
    assert chain_route(40, W=A + 2)[0] == -1
    assert chain_route(40, ts=24)[0] == -1 and b"samples_per_workgroup" in lib.mmdeer_last_error()
    assert lib.mmdeer_chain_route(None, None, 0) == -1
    a = _lib.ChainArgs()
    a.X, a.ldx, a.K0, a.rows, a.nseg = A, 256, 256, 40, 1
    s = a.seg[0]
    s.W, s.N, s.K, s.end_layer, s.nout, s.drop_site = A, 256, 256, 1, 256, -1
    assert lib.mmdeer_chain_route(C.byref(a), None, 0) == 1         # the answer without a buffer


def test_the_route_header_is_bound_like_the_others():
    assert {n: len(args) for n, _, args in _lib.ROUTE_SYMBOLS} == {"mmdeer_chain_route": 3, "mmdeer_step_chain_routes": 6}
    lib = _lib.load()
    for name, res, args in _lib.ROUTE_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
