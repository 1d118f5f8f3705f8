// optimizer_groups.hip — AdamW with parameter groups: one launch updates a flat slice of the parameter buffer that crosses any number
// of RUNS, each with its own learning-rate scale and weight decay, or frozen (optax.multi_transform over optax.adamw /
// optax.set_to_zero).  The element update is adamw_update.inc, the text of the kernels in optimizer.hip, included unchanged inside a
// device-side loop over the runs the slice touches: AdamW is elementwise, so on every run that is not frozen p, m, v and p_lp are bit
// for bit those of mic_adamw on that sub-range with hyper[0] pre-multiplied by the run's scale and the run's wd.
// A unit of its own (the Makefile's INC_UNIT_SRCS): tests/test_kernel_resources_cpu.py pins the kernel set of optimizer.hip.
#include "common.h"

#define ALIGNED16(p) ((reinterpret_cast<uintptr_t>(p) & 15) == 0)

// Every thread walks the table from the first run that ends behind the slice's begin (binary search: runs are sorted and gap-free) to
// the first that begins at or behind its end; the run's fields are wave-uniform loads.  Inside a run the whole grid strides over the
// run's float4s, as adamw_kernel<false> does over its buffer.  A frozen run is skipped before any of its bytes is addressed.
__global__ __launch_bounds__(256) void adamw_groups_kernel(long n_slice, long offset, float* __restrict__ p0, float* __restrict__ m0,
                                                           float* __restrict__ v0, const float* __restrict__ g0,
                                                           uint16_t* __restrict__ p_lp0, const float* __restrict__ hyper,
                                                           const mic_adamw_run* __restrict__ runs, int n_runs, float b1, float b2,
                                                           float omb1, float omb2, float eps, float gscale) {
  constexpr bool ROWS = false, ACC = false;
  const float* acc = nullptr;
  const uint8_t* row_flag = nullptr;
  const int row_f4 = 1, want = 0;
  const float t = hyper[1];
  const long s_end = offset + n_slice;
  int lo_r = 0, hi_r = n_runs;  // first run with end > offset
  while (lo_r < hi_r) {
    const int mid = (lo_r + hi_r) >> 1;
    if ((long)runs[mid].end <= offset) lo_r = mid + 1; else hi_r = mid;
  }
  for (int r = lo_r; r < n_runs; ++r) {
    const long rb = (long)runs[r].begin, re = (long)runs[r].end;
    if (rb >= s_end) break;
    if (runs[r].frozen) continue;
    const long lo = rb > offset ? rb : offset, hi = re < s_end ? re : s_end;
    if (hi <= lo) continue;
    const long n = hi - lo, d = lo - offset;
    float* __restrict__ p = p0 + d;
    float* __restrict__ m = m0 + d;
    float* __restrict__ v = v0 + d;
    const float* __restrict__ g = g0 + d;
    uint16_t* __restrict__ p_lp = p_lp0 ? p_lp0 + d : nullptr;
    const float lr = __fmul_rn(hyper[0], runs[r].lr_scale);  // one fp32 multiply: the float a caller of mic_adamw would pre-multiply
    const float wd = runs[r].wd;
#include "adamw_update.inc"
  }
}

extern "C" int mic_adamw_groups(int64_t n, int64_t offset, float* p, float* m, float* v, const float* g, void* p_lp, const float* hyper,
                                const mic_adamw_run* runs, int n_runs, double b1, double b2, double eps, float grad_scale, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && offset >= 0 && offset % 4 == 0 && p && m && v && g && hyper && runs && n_runs > 0,
            "mic_adamw_groups: bad args (n and offset must be multiples of 4, n_runs positive)");
  MIC_CHECK(ALIGNED16(p) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(g) && (reinterpret_cast<uintptr_t>(p_lp) & 7) == 0,
            "mic_adamw_groups: p, m, v and g must be 16-byte aligned (p_lp: 8-byte)");
  long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(adamw_groups_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)n, (long)offset, p, m, v, g, (uint16_t*)p_lp,
                     hyper, runs, n_runs, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, grad_scale);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
