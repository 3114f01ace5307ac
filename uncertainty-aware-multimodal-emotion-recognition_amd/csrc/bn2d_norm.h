// Device code shared by the forward and the backward of BatchNorm2d + ReLU on channels-last rows (bn2d.hip, bn2d_bwd.hip): the lane
// mapping and the normalisation itself.  The backward forms the ReLU mask and the pool's arg-max from the same expression as the
// forward stored its output from, so the two agree bit for bit.
#pragma once
#include "bn_fold.h"

namespace mmdeer {
namespace {

// thread t owns the four consecutive channels 4 * (t % (C / 4)) .. + 3 of every PAR-th row of its workgroup's share
struct Lane {
  int cq, par, PAR;
};
__device__ __forceinline__ Lane lane_of(int C) {
  const int CQ = C >> 2;   // a power of two
  return Lane{(int)threadIdx.x & (CQ - 1), (int)threadIdx.x / CQ, 256 / CQ};
}

// the normalisation of this thread's four channels: v = relu((x - mean) * rstd * gamma + beta)
struct Norm {
  f32x4 mean, rstd, gamma, beta;
  // A: an argument struct with mean, rstd, running, eps, gamma, beta
  template <typename A>
  __device__ __forceinline__ void load(const A& a, int cq) {
    mean = *reinterpret_cast<const f32x4*>(a.mean + 4 * cq);
    rstd = *reinterpret_cast<const f32x4*>(a.rstd + 4 * cq);
    if (a.running) {   // `rstd` holds the running variance
      rstd = f32x4{1.f / sqrtf(rstd.x + a.eps), 1.f / sqrtf(rstd.y + a.eps), 1.f / sqrtf(rstd.z + a.eps), 1.f / sqrtf(rstd.w + a.eps)};
    }
    gamma = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cq);
    beta = *reinterpret_cast<const f32x4*>(a.beta + 4 * cq);
  }
  __device__ __forceinline__ f32x4 xhat(const f32x4& x) const { return (x - mean) * rstd; }
  // a constant channel gives relu(beta) exactly: (x - mean) is an exact zero
  __device__ __forceinline__ f32x4 operator()(const f32x4& x) const { return relu4(fma4((x - mean) * rstd, gamma, beta)); }
};

}  // namespace
}  // namespace mmdeer
