// GEMM instantiations for trans_a = false, trans_b = true  (see gemm_kernel.inc)
#include "gemm_kernel.inc"

namespace mmdeer {

GEMM_REG_LAUNCHER(gemm_launch_nx_reg, false, true, GEMM_MODE_PAIRS_NX)

}  // namespace mmdeer
