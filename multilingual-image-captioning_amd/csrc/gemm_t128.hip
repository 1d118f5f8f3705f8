// 128x128x64 tiles, 8 waves per K-group (wave tile 64x32), one or two K-groups: instantiations of gemm_kernel.h
#include "gemm_kernel.h"
void launch_gemm_t128(const LaunchTable& tab, const GemmDecision& d, hipStream_t s) {
  if (d.kgroups == 2) launch_cfg<64, 32, 4, 64, 2>(tab, d, s);
  else launch_cfg<64, 32, 4, 64>(tab, d, s);
}
