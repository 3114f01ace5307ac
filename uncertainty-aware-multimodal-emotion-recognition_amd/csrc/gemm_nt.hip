// GEMM instantiations for trans_a = false, trans_b = false  (see gemm_kernel.inc)
#include "gemm_kernel.inc"

namespace mmdeer {

GEMM_REG_LAUNCHER(gemm_launch_nt_reg, false, false, GEMM_MODE_PAIRS_NT)

}  // namespace mmdeer
