"""The routes of mmdeer_gemm as a table: the arguments that select each kernel, the route line mmdeer_gemm_route must answer for
them, the epilogues, the launch plans and what each plan changes, the refusals -- and the layout of one call's buffers.  No GPU
is touched here: tests/test_gpu_gemm_routes.py runs the table on the device, tests/test_cpu_host.py asks the dry run alone."""
from mmdeer import _lib


def rup(x, m):
    return (x + m - 1) // m * m


def default_ld(extent, f32):
    """Default leading dimension: larger than the extent, a multiple of 8 for bf16 storage (16-byte chunks)."""
    return extent + 4 if f32 else rup(extent, 8) + 8


# ---------------------------------------------------------------------------------------------------------- the route table
# route name -> the arguments that select it, launch options, shapes (M, N, K) and `route`: the line mmdeer_gemm_route answers
# (without its tiles= part; a list parallel to `shapes` where the shapes differ, `route_epi` where an epilogue moves the call to
# another kernel).  The lines are written by hand from csrc/gemm.hip (gemm_route, pick_tile and the three *_takes predicates);
# both test files ASSERT them, so a changed threshold or predicate that moves a named route onto another kernel fails here.
# Leading dimensions default to default_ld(extent) (ld > extent everywhere), ldc to N + 4 (the 256-row forward kernel needs
# ldc % 8 == 0: N rounded up to 8, + 8).  Under bf16 compute the storage of an operand picks its loader source mode: fp32 = f32;
# bf16 with ld % 8 == 0 and extent % 8 == 0 = v16 (extent = K, or M / N when transposed); else v8.
NT, NX, TT = (0, 0), (0, 1), (1, 1)
ROUTES = {
    # register-staged NT kernel (gemm_group_kernel<.., false, false, ..>): fp32 compute; bf16 off the LDS-DMA kernels (a non-v16
    # operand, K % 64 != 0, or 128x128 tiles outside the 128x128 LDS-DMA condition).  Mode pairs (v16,v16), (f32,v16), (f32,v8), (v8,v8)
    "nt_f32_t0": dict(tr=NT, f32=1, a32=1, w32=1, tile=0, shapes=[(1, 4, 36), (63, 68, 100), (131, 132, 96)],
                      route="nt_reg 64x64 a=f32 b=f32"),
    "nt_f32_t1": dict(tr=NT, f32=1, a32=1, w32=1, tile=1, shapes=[(127, 68, 100), (129, 4, 36), (577, 196, 64)],
                      route="nt_reg 128x64 a=f32 b=f32"),
    "nt_f32_t2": dict(tr=NT, f32=1, a32=1, w32=1, tile=2, shapes=[(1, 132, 96), (129, 260, 100)], route="nt_reg 128x128 a=f32 b=f32"),
    "nt_bf16_v16v16_t0": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(1, 4, 96), (65, 68, 224), (131, 196, 40)],
                              route="nt_reg 64x64 a=v16 b=v16"),
    "nt_bf16_v16v16_t1": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 68, 96), (257, 132, 160)],
                              route="nt_reg 128x64 a=v16 b=v16"),
    "nt_bf16_v16v16_t2": dict(tr=NT, f32=0, a32=0, w32=0, tile=2, shapes=[(129, 132, 128), (1, 4, 96)],
                              route="nt_reg 128x128 a=v16 b=v16"),
    "nt_bf16_f32v16": dict(tr=NT, f32=0, a32=1, w32=0, tile=0, shapes=[(63, 68, 96), (131, 4, 128)], route="nt_reg 64x64 a=f32 b=v16"),
    "nt_bf16_f32v16_t2": dict(tr=NT, f32=0, a32=1, w32=0, tile=2, shapes=[(129, 132, 96)], route="nt_reg 128x128 a=f32 b=v16"),
    "nt_bf16_f32v8": dict(tr=NT, f32=0, a32=1, w32=0, tile=1, shapes=[(127, 68, 36), (131, 4, 100)], route="nt_reg 128x64 a=f32 b=v8"),
    "nt_bf16_v8v8": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(65, 68, 36), (1, 132, 100)], route="nt_reg 64x64 a=v8 b=v8"),
    "nt_bf16_v8v8_t2": dict(tr=NT, f32=0, a32=0, w32=0, tile=2, shapes=[(131, 260, 84)], route="nt_reg 128x128 a=v8 b=v8"),
    # register-staged NX kernel (dX = dY W with W stored [K][N]): fp32, or bf16 (v16,v16), (v16,v8 = N % 8 == 4)
    "nx_f32": dict(tr=NX, f32=1, a32=1, w32=1, tile=0, shapes=[(1, 4, 36), (65, 68, 100), (131, 196, 64)], route="nx_reg 64x64 a=f32 b=f32"),
    "nx_f32_t2": dict(tr=NX, f32=1, a32=1, w32=1, tile=2, shapes=[(129, 132, 96)], route="nx_reg 128x128 a=f32 b=f32"),
    "nx_bf16_v16v16": dict(tr=NX, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 136, 96), (1, 8, 64), (131, 264, 40)],
                           route="nx_reg 128x64 a=v16 b=v16"),
    "nx_bf16_v16v8": dict(tr=NX, f32=0, a32=0, w32=0, tile=0, shapes=[(65, 68, 96), (63, 4, 128), (131, 132, 40)],
                          route="nx_reg 64x64 a=v16 b=v8"),
    # register-staged TT kernel (dW = dY^T X, A stored [K][M], W stored [K][N]; M % 4 == 0): tiles 0 / 1 always, tile 2 with fp32
    # compute or off the DMA kernel.  bf16 (v16,v16), (v16,f32), (v16,v8 = N % 8 == 4)
    "tt_f32_t0": dict(tr=TT, f32=1, a32=1, w32=1, tile=0, shapes=[(4, 4, 1), (60, 68, 100), (132, 196, 37)], route="tt_reg 64x64 a=f32 b=f32"),
    "tt_f32_t2": dict(tr=TT, f32=1, a32=1, w32=1, tile=2, shapes=[(124, 132, 515), (260, 68, 64)], route="tt_reg 128x128 a=f32 b=f32"),
    "tt_bf16_v16v16": dict(tr=TT, f32=0, a32=0, w32=0, tile=0, shapes=[(8, 8, 3), (56, 72, 100), (136, 200, 37)],
                           route="tt_reg 64x64 a=v16 b=v16"),
    "tt_bf16_v16v16_t1": dict(tr=TT, f32=0, a32=0, w32=0, tile=1, shapes=[(120, 136, 260)], route="tt_reg 128x64 a=v16 b=v16"),
    "tt_bf16_v16f32": dict(tr=TT, f32=0, a32=0, w32=1, tile=1, shapes=[(136, 68, 100), (8, 4, 37)], route="tt_reg 128x64 a=v16 b=f32"),
    "tt_bf16_v16v8": dict(tr=TT, f32=0, a32=0, w32=0, tile=0, shapes=[(72, 68, 100), (136, 4, 64)], route="tt_reg 64x64 a=v16 b=v8"),
    # LDS-DMA NT kernel (gemm_nt_glds_kernel<BM, BN, NST, NW>): bf16 v16 x v16, K % 64 == 0, no split-K, no bias_grad.
    # tile 0: 64x64.  tile 1: 8-wave 128x64 up to 320 tiles (option nt8), 4-wave above; 128x128 (option nt128) when
    # N % 128 == 0, more than 320 tiles of 128x64 and 160..320 tiles of 128x128
    "glds_64x64": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(1, 4, 64), (63, 68, 128), (65, 196, 192), (131, 132, 64),
                                                                               (65, 68, 320)],   # 5 K-tiles: the ring's steady state
                       route="nt_glds 64x64 w4 a=v16 b=v16"),
    "glds_128x64_8w": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 68, 64), (129, 4, 128), (1031, 196, 64)],
                           route="nt_glds 128x64 w8 a=v16 b=v16"),
    "glds_128x64_4w": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(4093, 708, 64), (2689, 1028, 128)],
                           route="nt_glds 128x64 w4 a=v16 b=v16"),
    "glds_128x128": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(2561, 1280, 64), (2049, 2304, 128)],
                         route="nt_glds 128x128 w8 a=v16 b=v16"),
    # 256-row forward LDS-DMA kernel (gemm_nt256_kernel<BN>): tile 3, bf16 v16 x v16, K % 32 == 0, no Y / bias_grad / split-K,
    # C 16-byte aligned, ldc % 8 == 0.  BN = 192 (option nt192) when N % 192 == 0, t192 <= 256 and t192 > t256
    "nt256_256": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(1, 4, 32), (257, 260, 96), (255, 1028, 64),
                                                                              (257, 260, 160)],   # 5 K stages: the ring's steady state
                      route="nt256 256x256 a=v16 b=v16"),
    "nt256_192": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(777, 768, 96), (1, 768, 32)], route="nt256 256x192 a=v16 b=v16"),
    # weight-gradient LDS-DMA kernel (gemm_tt_dma_kernel<BM, BN, KG>): TT, bf16 A and W in 16-byte chunks (a half-valid last
    # chunk when ld >= extent rounded up to 8), K % 32 == 0, fp32 C 16-byte aligned, no epilogue but bias_grad / accumulate.
    # tile 3: 256x256; tile 2 with option dw_tile = 2: 128x128, K-split form (dw_kg = 2) when K % 64 == 0; tile 4: 256x128
    "tt_dma_256": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, shapes=[(8, 84, 32), (260, 84, 96), (520, 268, 1024)],
                       route="tt_dma 256x256 k1 a=v16 b=v16"),
    "tt_dma_128k2": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, shapes=[(8, 84, 64), (260, 132, 128), (136, 268, 1024)],
                         route="tt_dma 128x128 k2 a=v16 b=v16"),
    "tt_dma_128": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, shapes=[(260, 132, 96), (8, 4, 32)], route="tt_dma 128x128 k1 a=v16 b=v16"),
    "tt_dma_128_kg1": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, opts=dict(dw_kg=1), shapes=[(260, 132, 128)],
                           route="tt_dma 128x128 k1 a=v16 b=v16"),
    "tt_dma_256x128": dict(tr=TT, f32=0, a32=0, w32=0, tile=4, shapes=[(260, 84, 96), (516, 268, 256)],
                           route="tt_dma 256x128 k1 a=v16 b=v16"),
    "tt_auto": dict(tr=TT, f32=0, a32=0, w32=0, tile=-1, shapes=[(260, 132, 1024), (512, 84, 96)],   # pick_tile: dw_tile; K % 64
                    route=["tt_dma 128x128 k2 a=v16 b=v16", "tt_dma 128x128 k1 a=v16 b=v16"]),
    # fallbacks of tiles 3 / 4 where the DMA kernel does not apply (off it, N = 132 is read in 8-byte chunks)
    "fb_tt_k_ragged": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, shapes=[(136, 132, 100)], route="tt_reg 128x128 a=v16 b=v8"),   # K % 32
    "fb_tt4_k_ragged": dict(tr=TT, f32=0, a32=0, w32=0, tile=4, shapes=[(136, 132, 37)], route="tt_reg 128x128 a=v16 b=v8"),
    "fb_tt_c_unaligned": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, c_shift=2, shapes=[(136, 132, 96)],                        # C % 16
                              route="tt_reg 128x128 a=v16 b=v8"),
    "fb_nt_k_ragged": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(257, 132, 104)], route="nt_reg 128x64 a=v16 b=v16"),   # K % 32
    "fb_nt_c_unaligned": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, c_shift=2, shapes=[(257, 132, 128)],                       # C % 16
                              route="nt_glds 128x64 w8 a=v16 b=v16", route_epi=dict(bgrad="nt_reg 128x64 a=v16 b=v16")),
    "fb_nt_mask": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, epi_only=("Y32", "Y16"), shapes=[(257, 132, 64)],                 # Y
                       route="nt_glds 128x64 w8 a=v16 b=v16"),
    "fb_nt4": dict(tr=NT, f32=0, a32=0, w32=0, tile=4, shapes=[(257, 132, 96)], route="nt_reg 128x64 a=v16 b=v16"),   # 256x128 is dW only
}

# epilogues: name -> argument overrides.  NT / NX routes take the forward / dX ones, TT routes the weight-gradient ones.
EPI_FWD = {
    "plain": {},
    "bias_relu": dict(bias=1, relu=1),
    "drop0": dict(bias=1, relu=1, drop_site=4, drop_shift=0, p=0.3),
    "drop5": dict(drop_site=1, drop_shift=5, p=0.25),
    "regen": dict(regen_site=7, p=0.4),
    "Y32": dict(Y=1, y32=1, mask_scale=1.0 / 0.7),
    "Y16": dict(Y=1, y32=0, mask_scale=1.5),
    "acc": dict(accumulate=1, bias=1),
    "c16": dict(c32=0, bias=1, relu=1),
    "c16_drop0": dict(c32=0, bias=1, relu=1, drop_site=4, drop_shift=0, p=0.3),   # dropout on a bf16 C: per column ...
    "c16_drop5": dict(c32=0, drop_site=1, drop_shift=5, p=0.25),                  # ... and per 32 columns
    "bgrad": dict(bias_grad=1),
}
EPI_DW = {
    "plain": {},
    "bgrad": dict(bias_grad=1),
    "sk3": dict(bias_grad=1, splitk=3, dense_c=1),
    "sk8": dict(splitk=8, dense_c=1),
    "sk_big": dict(bias_grad=1, splitk=1000, dense_c=1),
    "acc": dict(accumulate=1, bias_grad=1),
}
REPEAT = ("plain", "bgrad", "sk3", "drop0", "Y16")     # epilogues also run twice: bitwise identical


def epilogues(name, r):
    if r.get("epi_only"):
        return {k: EPI_FWD[k] for k in r["epi_only"]}
    if r["tr"] == TT:
        e = dict(EPI_DW)
        if not name.startswith(("tt_dma", "fb_tt", "tt_auto")):
            e["c16_relu"] = dict(c32=0, relu=1)       # an epilogue on a register-staged dW
        return e
    e = dict(EPI_FWD)
    if name.startswith(("glds", "nt256")):
        for k in ("Y32", "Y16", "bgrad"):              # each of these moves the call off that kernel (see fb_nt_mask)
            e.pop(k)
    if r.get("c_shift"):
        for k in ("c16", "c16_drop0", "c16_drop5"):    # a bf16 C two elements off is not 8-byte aligned (a refusal)
            e.pop(k)
    return e


def spec(route, M, N, K, **kw):
    r = ROUTES[route]
    s = dict(M=M, N=N, K=K, ta=r["tr"][0], tw=r["tr"][1], f32=r["f32"], a32=r["a32"], w32=r["w32"], tile=r["tile"],
             c32=1, c_shift=r.get("c_shift", 0), bias=0, relu=0, drop_site=-1, drop_shift=0, regen_site=-1, p=0.0, Y=0,
             y32=1, mask_scale=1.0, accumulate=0, bias_grad=0, splitk=1, seed=1234, offset=5, offset_dev=None)
    s.update(kw)
    return s


def route_line(route, shape=0, epilogue=None):
    """The line (without tiles=) the dry run answers for shape number `shape` of the route under `epilogue`."""
    r = ROUTES[route]
    if epilogue in r.get("route_epi", {}):
        return r["route_epi"][epilogue]
    return r["route"] if isinstance(r["route"], str) else r["route"][shape]


def route_cases(route):
    """(spec, shape number, epilogue name) of every shape of the route under every epilogue it takes."""
    r = ROUTES[route]
    for i, (M, N, K) in enumerate(r["shapes"]):
        for ename, e in epilogues(route, r).items():
            yield spec(route, M, N, K, **e), i, ename


# a representative subset of the routes, re-run under every non-default launch-plan value
PLAN_ROUTES = ["nt_bf16_v16v16_t1", "glds_64x64", "glds_128x64_8w", "glds_128x64_4w", "glds_128x128", "nt256_256", "nt256_192",
               "tt_dma_256", "tt_dma_128k2", "tt_dma_256x128", "tt_auto", "tt_bf16_v16v16", "nx_bf16_v16v16", "nt_f32_t1"]
PLANS = [dict(glds=0), dict(nt8=0), dict(nt128=0), dict(nt192=0), dict(xcd=0), dict(dw_tile=3), dict(dw_tile=4), dict(dw_kg=1)]


def plan_cases(route):
    """(spec, shape number, epilogue name) of the route's first two shapes as test_launch_plans runs them."""
    r = ROUTES[route]
    for i, (M, N, K) in enumerate(r["shapes"][:2]):
        if r["tr"] == TT and not r["f32"]:
            # a transposed bf16 A with M % 8 == 4 is read in half-valid chunks by the weight-gradient DMA kernel only;
            # the plans that move the call off that kernel refuse it (REFUSALS: tt_v8_v16)
            M = rup(M, 8)
        for ename in (("bgrad", "sk3") if r["tr"] == TT else ("plain", "drop0")):
            yield spec(route, M, N, K, **(EPI_DW if r["tr"] == TT else EPI_FWD)[ename]), i, ename


def plan_route_line(plan, route, shape, s):
    """What the launch plan changes of route_line(route, shape), stated by hand.  Off the weight-gradient DMA kernel a transposed W
    with N % 8 == 4 is no longer read in 16-byte chunks (b=v8)."""
    line = route_line(route, shape)
    (opt, value), = plan.items()
    tt_reg = "tt_reg 128x128 a=v16 b=" + ("v16" if s["N"] % 8 == 0 else "v8")
    if opt == "glds":       # no LDS-DMA kernel: the register-staged one at the requested tile, 256-row tiles as 128x64 / 128x128
        if route.startswith("glds_"):
            return ("nt_reg 64x64" if ROUTES[route]["tile"] == 0 else "nt_reg 128x64") + " a=v16 b=v16"
        if route.startswith("nt256_"):
            return "nt_reg 128x64 a=v16 b=v16"
        if route.startswith("tt_dma_") or route == "tt_auto":
            return tt_reg
    if opt == "nt8" and route == "glds_128x64_8w":
        return line.replace(" w8 ", " w4 ")
    if opt == "nt128" and route == "glds_128x128":
        return "nt_glds 128x64 w4 a=v16 b=v16"
    if opt == "nt192" and route == "nt256_192":
        return "nt256 256x256 a=v16 b=v16"
    if opt == "dw_tile":    # the automatic tile follows the option; an explicit 128x128 request no longer names the DMA kernel
        if route == "tt_auto":
            return {3: "tt_dma 256x256 k1", 4: "tt_dma 256x128 k1"}[value] + " a=v16 b=v16"
        if ROUTES[route]["tr"] == TT and ROUTES[route]["tile"] == 2:
            return tt_reg
    if opt == "dw_kg":
        return line.replace(" k2 ", " k1 ")
    return line             # xcd, and every route a plan does not name


UNSPLITTABLE = {   # name: (route, arguments) of a problem whose outputs the split-K fold cannot take
    "ldc_wide_f32": ("tt_f32_t0", dict(M=60, N=68, K=515, ldc=76)),
    "ldc_wide_bf16": ("tt_bf16_v16v16_t1", dict(M=120, N=136, K=1024, ldc=144)),
    "ldc_wide_dma128": ("tt_dma_128k2", dict(M=260, N=132, K=1024, ldc=140)),
    "ldc_wide_dma256": ("tt_dma_256", dict(M=520, N=268, K=1024, ldc=276)),
    "c_unaligned": ("tt_f32_t2", dict(M=124, N=132, K=515, c_shift=2, dense_c=1)),
    "bias_grad_M130": ("nt_f32_t0", dict(M=130, N=68, K=1000, dense_c=1)),
    "bias_grad_M131": ("nt_f32_t1", dict(M=131, N=132, K=640, dense_c=1)),
}


# ------------------------------------------------------------------------------------------------------------------ refusals
def _set(**kw):
    return lambda s: s.update(kw)


def _args(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


# name: (route, (M, N, K), change of the spec before the buffers are built, change of the struct after, word(s) of the message).
# On the device every pointer stays a real allocation: a missing check must not launch on a made-up address.
REFUSALS = {
    "N_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(N=66), "N=66"),
    "K_mod4_A": ("nt_f32_t0", (64, 68, 66), None, None, "K=66"),
    "M_mod4_transA": ("tt_f32_t0", (62, 68, 64), None, None, "M=62"),
    "lda_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(lda=70), "leading dims"),
    "ldw_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(ldw=70), "leading dims"),
    "ldc_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(ldc=70), "leading dims"),
    "ldy_mod4": ("nt_f32_t0", (64, 68, 64), _set(Y=1), _args(ldy=70), "ldy"),
    "A_unaligned": ("nt_f32_t0", (64, 68, 64), _set(a_shift=2), None, "aligned"),
    "W_unaligned": ("nt_bf16_v16v16_t0", (64, 68, 64), _set(w_shift=4), None, "aligned"),
    "accumulate_bf16_C": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(c32=0), _args(accumulate=1), "accumulate"),
    "splitk_bias": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, bias_grad=1, dense_c=1), lambda a: setattr(a, "bias", a.bias_grad),
                    "split-K"),
    "splitk_relu": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, bias_grad=1, dense_c=1), _args(relu=1), "split-K"),
    "splitk_accumulate": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(accumulate=1), "split-K"),
    "splitk_drop": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(drop_site=2, dropout_p=0.5), "split-K"),
    "splitk_bf16_C": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(c_f32=0), "split-K"),
    "splitk_no_slab": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(slab=None), "slab"),
    "splitk_no_slab_wide_ldc": ("tt_f32_t0", (64, 68, 512), _set(splitk=3), _args(slab=None), "slab"),
    "f32_compute_bf16_A": ("nt_f32_t0", (64, 68, 64), _set(a32=0), None, "fp32 operands"),
    "f32_compute_bf16_W": ("nx_f32", (64, 68, 64), _set(w32=0), None, "fp32 operands"),
    "nt_v16_f32": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(w32=1), None, "not instantiated"),
    "nt_v8_v16": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(lda=100), None, "not instantiated"),
    "nt_v16_v8": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(ldw=100), None, "not instantiated"),
    "nt_v8_f32": ("nt_bf16_v16v16_t0", (64, 68, 36), _set(w32=1), None, "not instantiated"),
    "nx_f32_v16": ("nx_bf16_v16v16", (64, 72, 96), _set(a32=1), None, "not instantiated"),
    "nx_v8_v16": ("nx_bf16_v16v16", (64, 72, 36), None, None, "not instantiated"),
    "nx_v16_f32": ("nx_bf16_v16v16", (64, 72, 96), _set(w32=1), None, "not instantiated"),
    "tt_v8_v16": ("tt_bf16_v16v16", (68, 72, 96), None, None, "not instantiated"),     # M % 8 == 4 off the DMA kernels
    "tt_f32_v16": ("tt_bf16_v16v16", (64, 72, 96), _set(a32=1), None, "not instantiated"),
    "tt_half_valid_A_unaligned_C": ("tt_dma_256", (260, 84, 96), _set(c_shift=2), None, "not instantiated"),
    "transA_only": ("tt_f32_t0", (64, 68, 64), None, _args(trans_w=0), "trans_a=1, trans_b=0"),
    "lda_short": ("nt_f32_t0", (64, 68, 64), _set(lda=60), None, "lda=60"),
    "lda_short_transA": ("tt_f32_t0", (64, 68, 64), _set(lda=60), None, "lda=60"),
    "ldw_short": ("nt_f32_t0", (64, 68, 64), _set(ldw=60), None, "ldw=60"),
    "ldw_short_transW": ("nx_f32", (64, 68, 64), _set(ldw=64), None, "ldw=64"),
    "ldc_short": ("nt_f32_t0", (64, 68, 64), _set(ldc=64), None, "ldc=64"),
    "ldc_short_glds": ("glds_64x64", (64, 68, 64), _set(ldc=64), None, "ldc=64"),
    "ldy_short": ("nt_f32_t0", (64, 68, 64), _set(Y=1, ldy=64), None, "ldy=64"),
}


def refusal_spec(name):
    """(spec, change of the built struct or None, words of the message) of one REFUSALS entry."""
    route, (M, N, K), pre, post, words = REFUSALS[name]
    s = spec(route, M, N, K, bias_grad=int(ROUTES[route]["tr"] == TT))
    if pre:
        pre(s)
    return s, post, words


# -------------------------------------------------------------------------------------------------------- one call's buffers
class Layout:
    """Where one call's matrices sit inside their buffers, in elements: leading dimensions, C one canary row (+ c_shift) into its
    buffer, bias_grad 4 floats into its own, operands `a_shift` / `w_shift` into theirs, the split-K slab's slice."""

    def __init__(self, s):
        M, N, K = s["M"], s["N"], s["K"]
        self.a_rows, self.a_cols = (K, M) if s["ta"] else (M, K)
        self.w_rows, self.w_cols = (K, N) if s["tw"] else (N, K)
        self.lda = s.get("lda") or default_ld(self.a_cols, s["a32"])
        self.ldw = s.get("ldw") or default_ld(self.w_cols, s["w32"])
        if s.get("ldc"):
            self.ldc = s["ldc"]
        elif s.get("dense_c"):
            self.ldc = N
        else:
            self.ldc = rup(N, 8) + 8 if s["tile"] == 3 and not s["ta"] else N + 4
        self.ldy = s.get("ldy") or N + 4
        self.a_shift, self.w_shift = s.get("a_shift", 0), s.get("w_shift", 0)
        self.c_off = self.ldc + s["c_shift"]                 # one canary row above C
        self.bg_off = 4
        # the library may use min(splitk, K-tiles) slices of M*N + M floats (rounded up to 4)
        self.slice = rup(M * N + M, 4)
        self.slices = min(s["splitk"], -(-K // (32 if s["f32"] else 64)))

    def args(self, s, A, W, C, bias=None, bias_grad=None, Y=None, slab=None, stream=None):
        """mmdeer_gemm_args of the spec, given the base address of each buffer (None where the spec does not use it)."""
        def at(base, elems, f32):
            return base + elems * (4 if f32 else 2)
        return _lib.gemm_args(
            A=at(A, self.a_shift, s["a32"]), W=at(W, self.w_shift, s["w32"]), C=at(C, self.c_off, s["c32"]),
            bias=bias if s["bias"] else None, bias_grad=at(bias_grad, self.bg_off, 1) if s["bias_grad"] else None,
            Y=Y if s["Y"] else None, M=s["M"], N=s["N"], K=s["K"], lda=self.lda, ldw=self.ldw, ldc=self.ldc,
            ldy=self.ldy if s["Y"] else 0, a_f32=s["a32"], w_f32=s["w32"], c_f32=s["c32"], y_f32=s["y32"], trans_a=s["ta"],
            trans_w=s["tw"], relu=s["relu"], accumulate=s["accumulate"], compute_f32=s["f32"], tile=s["tile"],
            drop_site=s["drop_site"], drop_shift=s["drop_shift"], regen_site=s["regen_site"], dropout_p=s["p"],
            mask_scale=s["mask_scale"], seed=s["seed"], offset=s["offset"], offset_dev=s["offset_dev"], splitk=s["splitk"],
            slab=slab if s["splitk"] > 1 else None, stream=stream)


def dry_run(args):
    """(return code, lines) of mmdeer_gemm_route on an argument struct."""
    import ctypes as C
    out = C.create_string_buffer(512)
    rc = _lib.load().mmdeer_gemm_route(C.byref(args), out, len(out))
    return rc, out.value.decode().split("\n") if out.value else []


def without_tiles(line):
    return line.rsplit(" tiles=", 1)[0]
