/* mmdeer -- C ABI of the layer chains' route queries (csrc/chain.hip: chain_route): which kernel a chain launch would run.  A
 * companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding), exported by the same library and covered
 * by the same MMDEER_ABI_VERSION.  Both calls are dry runs in the style of mmdeer_gemm_route: host code only, no GPU touched, no operand
 * pointer dereferenced; a refused call returns -1 and leaves its reason in mmdeer_last_error(). */
#ifndef MMDEER_ROUTES_H_
#define MMDEER_ROUTES_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmdeer_chain_args mmdeer_chain_args;     /* include/mmdeer.h */

/* Dry run of mmdeer_chain: every check it makes before its launch, touching no GPU and dereferencing no operand pointer.  Writes
 * "<kernel> workgroups=<n>" into out[cap] (NUL-terminated, truncated to fit): kernel s16 (16-sample workgroups, 4-deep weight ring),
 * s16_d2 / s16_d8 (the same under option chain_depth = 2 / 8), s32 (32-sample workgroups).  Returns 1 (rows = 0: 0, nothing written), or
 * -1 with the message of mmdeer_last_error() exactly where mmdeer_chain would refuse. */
int mmdeer_chain_route(const mmdeer_chain_args* a, char* out, int cap);
/* The chain launches of one single-call training step of Stack C (mmdeer_forward, then mmdeer_backward with phase = 0 and no g_fused)
 * at this batch under the current options, one line "<launch> <kernel>" each, in launch order: launch F1-F6 (F2-F6 without the input
 * chain), F9-F17 (F9-F18 with chain_nigf), B1-B10 (B2-B10 without the NIG prologue), B13-B17; kernel as above.  `targets`: the step
 * computes the loss (only then can the backward chain carry the NIG prologue).  Returns the number of chain launches (0: the batch
 * takes the launch-by-launch plan); touches no GPU. */
int mmdeer_step_chain_routes(int batch, int compute_f32, int inputs_bf16, int targets, char* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
