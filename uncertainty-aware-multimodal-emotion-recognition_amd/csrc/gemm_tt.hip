// GEMM instantiations for trans_a = true, trans_b = true  (see gemm_kernel.inc)
#include "gemm_kernel.inc"

namespace mmdeer {

GEMM_REG_LAUNCHER(gemm_launch_tt_reg, true, true, GEMM_MODE_PAIRS_TT)

}  // namespace mmdeer
