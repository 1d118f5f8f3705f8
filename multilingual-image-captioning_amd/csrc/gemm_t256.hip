// 256x256x64 tiles, 8 waves (wave tile 128x64): instantiations of gemm_kernel.h
#include "gemm_kernel.h"
void launch_gemm_t256(const LaunchTable& tab, const GemmDecision& d, hipStream_t s) { launch_cfg<128, 64, 4, 64>(tab, d, s); }
