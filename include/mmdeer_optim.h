/* mmdeer -- C ABI of the optimiser step over ANY list of fp32 tensors (csrc/optim_multi.hip): global-norm gradient clipping +
 * AdamW for parameters that train through autograd into ordinary .grad tensors, where mmdeer_adamw_step and mmdeer_adamw_flat
 * (mmdeer.h) serve one model's flat gradient buffer each.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the
 * ctypes binding), exported by the same library and covered by the same MMDEER_ABI_VERSION.
 *
 * THE STEP, stated once.  Over the listed tensors, with gs = grad_scale and every scalar the float32 value passed:
 *   norm = |gs| sqrt(sum g^2)                                         the 2-norm of gs * g over ALL listed tensors (fp32, fixed order)
 *   clip = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1      torch's clip_grad_norm_
 *   g'   = g (clip gs)
 *   per tensor, with its class's lr, weight_decay and step, bc1 = 1 - beta1^step, bc2 = 1 - beta2^step:
 *   p   *= 1 - lr weight_decay                                        torch.optim.AdamW's decoupled decay
 *   m    = m beta1 + g' (1 - beta1),  v = v beta2 + g' g' (1 - beta2)
 *   p   -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * as separate fp32 operations in this order (no contraction; csrc/optim.h: adamw_update4, the element update of the two older
 * entries).  The bias corrections are formed on the host (powf), never per element.  After the update element i of the parameter is
 * also stored at mirror[i] where the tensor has a mirror: as fp32, or as bf16 rounded to nearest even.  A tensor that is to be
 * skipped (torch: grad is None) is simply not listed: it is neither read nor written and does not enter the norm.
 *
 * TENSORS.  Any contiguous fp32 tensor whose pointers are 4-byte aligned (a bf16 mirror: 2-byte); views at odd element offsets are
 * taken.  Where a tensor's gradient, moments and mirror sit at the same offset modulo 4 elements as its parameter, the 16-byte
 * aligned body of the tensor moves in 16-byte accesses per lane (a bf16 mirror in 8-byte stores) with a scalar head and tail; a
 * tensor where they do not moves element by element, to the same bits.  count == 0 is skipped.
 *
 * CLASSES carry what differs between tensors per step: lr, weight_decay and the step count (torch counts steps per parameter: a
 * parameter left out of a step does not advance).  At most MMDEER_ADAMW_MULTI_MAX_CLASSES ride in the kernel arguments; beta1,
 * beta2 and eps are per call.
 *
 * THE TABLE.  The tensor records do not fit the kernel arguments, so the kernels read them from device memory: `table`, at least
 * mmdeer_adamw_multi_table_bytes(tensors, ntensors) bytes, 16-byte aligned, owned by the caller.  The library derives the table
 * from the host records (pointers, counts, moment offsets, class indices, and the chunk index of MMDEER_ADAMW_MULTI_CHUNK elements
 * per chunk); no per-step scalar is in it.  The caller passes the host records on EVERY call (they are validated on every call) and
 * says with `upload` whether the device copy must be written: nonzero on the first call and whenever a record or one of
 * exp_avg / exp_avg_sq changed (a gradient reallocated at another address, another class index, a tensor more or fewer), zero
 * otherwise -- an ordinary step uploads nothing.  An upload is a copy on `stream` from memory of the library's own followed by a
 * wait for that stream before the call returns: blocking, and the library alone keeps the host memory of the copy alive; the
 * caller's records are not read after the call returns.  With upload == 0 the caller vouches that the table holds the upload of
 * these very records.  mmdeer_adamw_multi_uploads counts the uploads of the process.
 *
 * TWO LAUNCHES on `stream`, no host synchronisation without an upload, no atomics: two calls from the same state store the same bits.
 *   1  sum-of-squares partials over the listed gradients: chunk c goes to workgroup c mod grid, lane -> wave -> block -> scratch
 *   2  every workgroup folds the partials itself in a fixed order, forms clip, (workgroup 0) writes norm to grad_norm, updates
 *      its chunks and writes the mirrors
 *
 * REFUSALS return -1 with mmdeer_last_error and write nothing: a NULL args / tensors / moment buffer / scratch / table, a table
 * smaller than mmdeer_adamw_multi_table_bytes or not 16-byte aligned, ntensors < 0, nclasses outside 1 .. MAX_CLASSES, a class with
 * step < 1, a non-finite or non-positive lr, a negative or non-finite weight_decay; eps non-finite or <= 0, a beta outside [0, 1),
 * a non-finite grad_scale or max_grad_norm; per tensor a NULL or misaligned param / grad, a misaligned mirror, count < 0, a class
 * index out of range, a moment range [moment_off, moment_off + count) that passes moment_elems or overlaps another tensor's.
 *
 * THE CAPTURABLE STEP.  include/mmdeer_graph.h declares mmdeer_adamw_multi_dev: the same step with the classes' lr, weight decay and
 * step COUNT in device memory and a table upload made of launches alone, for a stream capture. */
#ifndef MMDEER_OPTIM_H_
#define MMDEER_OPTIM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDEER_ADAMW_MULTI_MAX_CLASSES 16
#define MMDEER_ADAMW_MULTI_CHUNK 1024
/* fp32 elements of `scratch`: the sum-of-squares partials */
#define MMDEER_ADAMW_MULTI_SCRATCH 2048

typedef struct mmdeer_adamw_multi_tensor {
  float* param;             /* fp32, count elements, updated in place */
  const float* grad;        /* fp32, count elements */
  void* mirror;             /* NULL, or count elements of fp32 (mirror_f32 != 0) / bf16 that take the updated parameter */
  long long count;
  long long moment_off;     /* element offset of this tensor's moments in exp_avg / exp_avg_sq */
  int32_t cls;              /* index into classes */
  int32_t mirror_f32;
} mmdeer_adamw_multi_tensor;

typedef struct mmdeer_adamw_multi_class {
  float lr, weight_decay;
  int32_t step;             /* >= 1: the step this call performs for the tensors of the class */
  int32_t reserved;
} mmdeer_adamw_multi_class;

typedef struct mmdeer_adamw_multi_args {
  const mmdeer_adamw_multi_tensor* tensors;       /* host records */
  int32_t ntensors, nclasses;
  mmdeer_adamw_multi_class classes[MMDEER_ADAMW_MULTI_MAX_CLASSES];
  float* exp_avg; float* exp_avg_sq;              /* flat fp32 moment buffers of moment_elems elements, owned by the caller */
  long long moment_elems;
  void* table;                                    /* device memory, table_bytes bytes */
  long long table_bytes;
  int32_t upload;                                 /* nonzero: write the table from the records before the launches */
  int32_t reserved;
  float* scratch;                                 /* device, MMDEER_ADAMW_MULTI_SCRATCH floats */
  float* grad_norm;                               /* device scalar or NULL: the norm before clipping */
  float beta1, beta2, eps, max_grad_norm, grad_scale;
  void* stream;
} mmdeer_adamw_multi_args;
int mmdeer_adamw_multi(const mmdeer_adamw_multi_args* a);
/* bytes of the device table for these records; -1 for records the call refuses (NULL with ntensors > 0, a negative count, ...) */
long long mmdeer_adamw_multi_table_bytes(const mmdeer_adamw_multi_tensor* tensors, int32_t ntensors);
/* how many table uploads mmdeer_adamw_multi has made in this process */
long long mmdeer_adamw_multi_uploads(void);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_OPTIM_H_ */
