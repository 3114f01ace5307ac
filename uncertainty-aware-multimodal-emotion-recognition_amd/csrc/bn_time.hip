// nn.BatchNorm1d(512) over the rows of an [R][512] activation matrix, for the temporal video encoder (reference
// src/models/encoders.py:450-459): the statistics are per channel over all R = T * B rows -- the library's only normalisation
// across rows beside the frame backbone's (bn2d.hip).  The method, the lane mapping and the statistics and backward kernels are
// bn_rows.h's, at C = 512 (two rows of a block in flight); this file holds what is this operator's: the apply kernel with the dropout
// draw, g = dout * (out > 0) * mask_scale of the backward, and the leading dimensions.
#include "bn_rows.h"

namespace mmdeer {
namespace {

constexpr int BN_C = 512;          // channels

template <bool F32>
__global__ __launch_bounds__(256) void bn_apply_kernel(mmdeer_bn_time_args a, DropCtx dc, int rpb) {
  const Lane l = lane_of(BN_C);
  const int cq = l.cq, r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, a.R);
  Norm norm;
  norm.load(a, cq);
  const bool drop = a.drop_site >= 0 && a.dropout_p > 0.f;
  const unsigned dkey = drop ? drop_key(dc, a.drop_site) : 0u;
  bn_rows<4>(r0 + l.par, r1, l.PAR, [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.ld_x + 4 * cq); },
             [&](int r, const f32x4& x) __attribute__((always_inline)) {
               f32x4 v = norm.affine(x);
               if (a.relu) v = relu4(v);
               if (drop) v = drop4(v, ((unsigned)r * 0x9E3779B1u) ^ dkey, (unsigned)(4 * cq), 0, dc);
               st4<F32>(a.out, (long long)r * a.ld_out + 4 * cq, v);
             });
}

// the backward's gradient functor (bn_rows.h): g = dout * (out > 0) * mask_scale, or dout where no `out` is given
template <bool F32>
struct TimeGrad {
  using Args = mmdeer_bn_time_args;
  Stats st;
  const Args* a;
  int cq;

  __device__ __forceinline__ void init(const Args& a_, int cq_) {
    st.load(a_, cq_);
    a = &a_; cq = cq_;
  }
  __device__ __forceinline__ f32x4 operator()(int r, f32x4& xh) const {
    f32x4 g = ld4<F32>(a->dout, (long long)r * a->ld_dout + 4 * cq);
    if (a->out) {
      const f32x4 o = ld4<F32>(a->out, (long long)r * a->ld_out + 4 * cq);
      const float ms = a->mask_scale;
      g = f32x4{o.x > 0.f ? g.x * ms : 0.f, o.y > 0.f ? g.y * ms : 0.f, o.z > 0.f ? g.z * ms : 0.f, o.w > 0.f ? g.w * ms : 0.f};
    }
    xh = st.xhat(ld4<F32>(a->x, (long long)r * a->ld_x + 4 * cq));
    return g;
  }
  __device__ __forceinline__ f32x4 scale() const { return *reinterpret_cast<const f32x4*>(a->gamma + 4 * cq) * st.rstd; }
  __device__ __forceinline__ void store(int r, const f32x4& dx) const { st4<F32>(a->dx, (long long)r * a->ld_dx + 4 * cq, dx); }
};

int check_bn(const mmdeer_bn_time_args* a, const char* op) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->C == BN_C, "%s: C must be %d (got %d)", op, BN_C, a->C);
  MMDEER_CHECK(a->R >= 0, "%s: bad row count R=%d", op, a->R);
  return 0;
}
bool act_ok(const mmdeer_bn_time_args* a, const void* p, int ld) {
  return p && al16(p) && ld >= BN_C && ld % (a->act_f32 ? 4 : 8) == 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn_time_stats(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_stats"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x), "bn_time_stats: x must be non-NULL, 16-byte aligned, ld_x >= %d and a multiple of 16 bytes", BN_C);
  return bn_launch_stats(a, "bn_time_stats", a->x, a->ld_x, a->R);
}

int mmdeer_bn_time_apply(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_apply"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x) && act_ok(a, a->out, a->ld_out),
               "bn_time_apply: x and out must be non-NULL, 16-byte aligned, ld >= %d and a multiple of 16 bytes", BN_C);
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->beta && al16(a->mean) && al16(a->rstd) && al16(a->gamma) && al16(a->beta),
               "bn_time_apply: mean, rstd, gamma, beta must be non-NULL and 16-byte aligned");
  MMDEER_CHECK(a->dropout_p >= 0.f && a->dropout_p < 1.f, "bn_time_apply: dropout_p must be in [0, 1)");
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, a->offset_dev);
  const RowPlan p = bn_row_plan(a->R);
  MMDEER_LAUNCH_ACT(bn_apply_kernel, a->act_f32, dim3(p.nblk), dim3(256), (hipStream_t)a->stream, *a, dc, p.rpb);
  return 0;
}

int mmdeer_bn_time_bwd(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_bwd"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x) && act_ok(a, a->dout, a->ld_dout) && act_ok(a, a->dx, a->ld_dx) &&
               (!a->out || act_ok(a, a->out, a->ld_out)),
               "bn_time_bwd: x, dout, dx (and out) must be non-NULL, 16-byte aligned, ld >= %d and a multiple of 16 bytes", BN_C);
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->dgamma && a->dbeta && a->scratch && al16(a->mean) && al16(a->rstd) &&
               al16(a->gamma) && al16(a->dgamma) && al16(a->dbeta) && al16(a->scratch),
               "bn_time_bwd: mean, rstd, gamma, dgamma, dbeta, scratch must be non-NULL and 16-byte aligned");
  return a->act_f32 ? bn_launch_bwd<TimeGrad<true>, 4>(*a, a->R) : bn_launch_bwd<TimeGrad<false>, 4>(*a, a->R);
}

}  // extern "C"
