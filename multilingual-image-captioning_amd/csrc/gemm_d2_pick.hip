// gemm_d2_pick.hip — gemm_d2_kernel<2>: the two-blocks-per-CU 256 x 128 kernel of gemm_d2.hip with the scorer's epilogue (softmax
// partials and each row's picked value, C stored only where the caller passes one: mic_gemm_args.pick_col / pick_out).  The kernel's
// text is gemm_d2.hip's — K loop, tiling and accumulation order of <1> —; this unit holds the one instantiation, so that
// gemm_d2.hip's own object and resource listing stay what they were (table: tests/golden/kernel_resources_units_score.json).
#define MIC_D2_PICK_UNIT
#include "gemm_d2.hip"
