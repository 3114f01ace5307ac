/* mmdeer -- C ABI of the device-resident dropout step for the three single operators of mmdeer.h that take (seed, offset) BY VALUE:
 * mmdeer_dropout_mask, mmdeer_trimodal_attn_fwd and mmdeer_trimodal_attn_bwd.  Every other launch of the audio, video and frame
 * encoders, the fusion modules and the DEER head carries its step in an argument struct with an `offset_dev` field; these three were
 * what kept a training step through those modules from being replayed as a HIP graph (mmdeer/train_graph.py).  A companion of
 * mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding), exported by the same library and covered by the same
 * MMDEER_ABI_VERSION.  It continues include/mmdeer_graph.h, which states the counter for the BERT trunk's entries; it is a header of
 * its own because that header's list of entries is closed.
 *
 * Each entry is mmdeer_<operator>_dev(<the plain entry's arguments>, offset_dev): the LAST argument points at ONE uint64_t in device
 * memory, 8-byte aligned (anything else is refused, before any launch, whatever dropout_p is).  The effective step is
 * offset + *offset_dev (modulo 2^64), read on the device when the kernel runs: a captured graph that bumps the counter between replays
 * draws fresh masks from unchanged kernel arguments.  The host never dereferences the pointer and no launch writes the counter.
 * offset_dev == NULL IS the plain entry: one kernel text per operator (csrc/rowops.hip: dropout_mask_kernel; csrc/attention.hip:
 * tri_attn_fwd_kernel, tri_attn_bwd_kernel), in which every wave forms key(seed, offset + *offset_dev, site) once, before its first
 * element (csrc/common.h: drop_key).  Conventions and refusals are the plain entries'.  The counter is not read where no mask is
 * drawn from a step: mmdeer_dropout_mask_dev with dropout_p <= 0 (it stores the plain entry's bits at `offset`), the
 * attention pair with dropout_p <= 0 or training == 0. */
#ifndef MMDEER_DROP_DEV_H_
#define MMDEER_DROP_DEV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int mmdeer_dropout_mask_dev(int site, int rows, int cols, float dropout_p, uint64_t seed, uint64_t offset,
                            unsigned char* out, void* stream, const uint64_t* offset_dev);
int mmdeer_trimodal_attn_fwd_dev(const void* qkv, void* obar, float* probs, float* attn_w, float* av_w, int B,
                                 int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream,
                                 const uint64_t* offset_dev);
int mmdeer_trimodal_attn_bwd_dev(const void* qkv, const void* dobar, const float* probs, void* dqkv, int B,
                                 int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream,
                                 const uint64_t* offset_dev);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_DROP_DEV_H_ */
