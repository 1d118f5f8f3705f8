// optimizer.hip — the optimizer step over the flat fp32 parameter buffer: fused AdamW (whole buffer, or the flagged rows of the tied
// embedding), gradient accumulation (the running fp32 sum, and AdamW on g + acc), and global-norm gradient clipping (a sum of
// squares with a fixed summation order, the kernel that turns it into (norm, coefficient), and AdamW with its gradient scale read
// from device memory, so the host never waits for the norm).  The three AdamW kernels share one text, adamw_update.inc.
#include "common.h"

#define SUMSQ_MAX_BLOCKS 1024  // ~4 blocks per CU: one slot per block, so a step of a few dozen buckets leaves tens of thousands of slots
#define ALIGNED16(p) ((reinterpret_cast<uintptr_t>(p) & 15) == 0)

// ------------------------------------------------------------------ fused AdamW over the flat parameter buffer (K15)
// ROWS: the buffer is [rows][width] and only the rows with (row_flag[row] != 0) == want are updated — the tied embedding's
// AdamW in two passes (mic_adamw_rows): AdamW is elementwise, so the split is exact.
template <bool ROWS>
__global__ __launch_bounds__(256) void adamw_kernel(long n, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                    const float* __restrict__ g, uint16_t* __restrict__ p_lp,
                                                    const float* __restrict__ hyper, float b1, float b2, float omb1, float omb2,
                                                    float eps, float wd, float gscale, const uint8_t* __restrict__ row_flag,
                                                    int row_f4, int want) {
  constexpr bool ACC = false;
  const float* acc = nullptr;
  const float lr = hyper[0], t = hyper[1];
#include "adamw_update.inc"
}

// AdamW on g' = fp32(g + acc): the final micro-step of an accumulation reads the running sum itself instead of a separate
// 12 B/element pass in front of the update.  The sum is rounded to fp32 BEFORE gscale is applied, so the result is bit for bit
// adamw_kernel's on a pre-summed gradient.
template <bool ROWS>
__global__ __launch_bounds__(256) void adamw_acc_kernel(long n, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, const float* __restrict__ acc,
                                                        uint16_t* __restrict__ p_lp, const float* __restrict__ hyper, float b1, float b2,
                                                        float omb1, float omb2, float eps, float wd, float gscale,
                                                        const uint8_t* __restrict__ row_flag, int row_f4, int want) {
  constexpr bool ACC = true;
  const float lr = hyper[0], t = hyper[1];
#include "adamw_update.inc"
}

// AdamW with the gradient scale read from device memory: adamw_kernel / adamw_acc_kernel with gscale = *coef, so p, m, v and p_lp are
// bit for bit those of mic_adamw / mic_adamw_acc called with that float.
template <bool ACC>
__global__ __launch_bounds__(256) void adamw_clip_kernel(long n, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ g, const float* __restrict__ acc,
                                                         uint16_t* __restrict__ p_lp, const float* __restrict__ hyper,
                                                         const float* __restrict__ coef, float b1, float b2, float omb1, float omb2,
                                                         float eps, float wd) {
  constexpr bool ROWS = false;
  const uint8_t* row_flag = nullptr;
  const int row_f4 = 1, want = 0;
  const float lr = hyper[0], t = hyper[1], gscale = coef[0];
#include "adamw_update.inc"
}

// what the five mic_adamw* launches share: the grid (one float4 per thread, at most 8192 blocks) and the fp32 constants b1, b2,
// 1 - b1, 1 - b2, eps, wd of the entry point's doubles, the differences formed in double before they are rounded
static dim3 adamw_grid(long n) { long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192; return dim3((int)nb); }
#define ADAMW_CONSTS (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd

extern "C" int mic_adamw(int64_t n, float* p, float* m, float* v, const float* g, void* p_lp, const float* hyper, double b1,
                         double b2, double eps, double wd, float grad_scale, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && p && m && v && g && hyper, "mic_adamw: bad args (n must be a multiple of 4)");
  hipLaunchKernelGGL(adamw_kernel<false>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, (uint16_t*)p_lp, hyper,
                     ADAMW_CONSTS, grad_scale, (const uint8_t*)nullptr, 1, 0);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

extern "C" int mic_adamw_rows(int64_t rows, int width, const uint8_t* row_flag, int want, float* p, float* m, float* v, const float* g,
                              void* p_lp, const float* hyper, double b1, double b2, double eps, double wd, float grad_scale, void* stream) {
  MIC_CHECK(rows > 0 && width > 0 && width % 4 == 0 && row_flag && p && m && v && g && hyper, "mic_adamw_rows: bad args (width must be a multiple of 4)");
  const long n = (long)rows * width;
  hipLaunchKernelGGL(adamw_kernel<true>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, n, p, m, v, g, (uint16_t*)p_lp, hyper,
                     ADAMW_CONSTS, grad_scale, row_flag, width / 4, want);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

extern "C" int mic_adamw_acc(int64_t n, float* p, float* m, float* v, const float* g, const float* acc, void* p_lp, const float* hyper,
                             double b1, double b2, double eps, double wd, float grad_scale, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && p && m && v && g && acc && hyper, "mic_adamw_acc: bad args (n must be a multiple of 4)");
  hipLaunchKernelGGL(adamw_acc_kernel<false>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, acc, (uint16_t*)p_lp, hyper,
                     ADAMW_CONSTS, grad_scale, (const uint8_t*)nullptr, 1, 0);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
extern "C" int mic_adamw_rows_acc(int64_t rows, int width, const uint8_t* row_flag, int want, float* p, float* m, float* v, const float* g,
                                  const float* acc, void* p_lp, const float* hyper, double b1, double b2, double eps, double wd,
                                  float grad_scale, void* stream) {
  MIC_CHECK(rows > 0 && width > 0 && width % 4 == 0 && row_flag && p && m && v && g && acc && hyper,
            "mic_adamw_rows_acc: bad args (width must be a multiple of 4)");
  const long n = (long)rows * width;
  hipLaunchKernelGGL(adamw_acc_kernel<true>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, n, p, m, v, g, acc, (uint16_t*)p_lp, hyper,
                     ADAMW_CONSTS, grad_scale, row_flag, width / 4, want);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

extern "C" int mic_adamw_clip(int64_t n, float* p, float* m, float* v, const float* g, const float* acc, void* p_lp, const float* hyper,
                              const float* coef, double b1, double b2, double eps, double wd, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && p && m && v && g && hyper && coef, "mic_adamw_clip: bad args (n must be a multiple of 4)");
  MIC_CHECK(ALIGNED16(p) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(g) && ALIGNED16(acc) && (reinterpret_cast<uintptr_t>(p_lp) & 7) == 0,
            "mic_adamw_clip: p, m, v, g and acc must be 16-byte aligned (p_lp: 8-byte)");
  if (acc) hipLaunchKernelGGL(adamw_clip_kernel<true>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, acc, (uint16_t*)p_lp,
                              hyper, coef, ADAMW_CONSTS);
  else hipLaunchKernelGGL(adamw_clip_kernel<false>, adamw_grid(n), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, (const float*)nullptr,
                          (uint16_t*)p_lp, hyper, coef, ADAMW_CONSTS);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

// ------------------------------------------------------------------ gradient accumulation (N micro-batches per AdamW step)
// dst = src (INIT) or dst = dst + src: one IEEE fp32 add per element, 16-B loads and stores, grid-stride
template <bool INIT>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(long n4, float* __restrict__ dst, const float* __restrict__ src) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
    float4 s = reinterpret_cast<const float4*>(src)[e];
    if constexpr (!INIT) {
      const float4 d = reinterpret_cast<const float4*>(dst)[e];
      s = make_float4(d.x + s.x, d.y + s.y, d.z + s.z, d.w + s.w);
    }
    reinterpret_cast<float4*>(dst)[e] = s;
  }
}
extern "C" int mic_grad_accumulate(int64_t n, float* dst, const float* src, int init, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && dst && src, "mic_grad_accumulate: bad args (n must be a multiple of 4)");
  long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
  if (init) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)(n / 4), dst, src);
  else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)(n / 4), dst, src);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

// ------------------------------------------------------------------ sum of squares of g (or of fp32(g + acc)), one partial per block
// Fixed order, no atomics: thread-private fp32 sums over a grid-stride walk (one per float4 component), the VALU/DPP butterfly inside
// each wave, the four waves through LDS as (w0 + w1) + (w2 + w3).  Block b plain-stores partials[b]: every slot the finaliser reads
// is written by this launch, whatever the buffer held.  The square is rounded to fp32 before it is added (__fmul_rn / __fadd_rn: no
// contraction), and with ACC the term is the fp32 sum adamw_acc_kernel forms before it scales.
template <bool ACC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(long n4, const float* __restrict__ g, const float* __restrict__ acc,
                                                         float* __restrict__ partials) {
  __shared__ float red[4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
    float4 x = reinterpret_cast<const float4*>(g)[e];
    if constexpr (ACC) {
      const float4 a = reinterpret_cast<const float4*>(acc)[e];
      x = make_float4(__fadd_rn(x.x, a.x), __fadd_rn(x.y, a.y), __fadd_rn(x.z, a.z), __fadd_rn(x.w, a.w));
    }
    s[0] = __fadd_rn(s[0], __fmul_rn(x.x, x.x));
    s[1] = __fadd_rn(s[1], __fmul_rn(x.y, x.y));
    s[2] = __fadd_rn(s[2], __fmul_rn(x.z, x.z));
    s[3] = __fadd_rn(s[3], __fmul_rn(x.w, x.w));
  }
  const float w = wave_sum(__fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = __fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3]));
}
// the launch geometry of mic_grad_sumsq, and with it the number of slots a call over n elements writes
extern "C" int64_t mic_grad_sumsq_slots(int64_t n) {
  if (n <= 0) return 0;
  const int64_t nb = ((n + 3) / 4 + 255) / 256;
  return nb > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : nb;
}
extern "C" int mic_grad_sumsq(int64_t n, const float* g, const float* acc, float* partials, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && g && partials, "mic_grad_sumsq: bad args (n must be a multiple of 4)");
  MIC_CHECK(ALIGNED16(g) && ALIGNED16(acc), "mic_grad_sumsq: g and acc must be 16-byte aligned");
  const int nb = (int)mic_grad_sumsq_slots(n);
  if (acc) hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (long)(n / 4), g, acc, partials);
  else hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (long)(n / 4), g, (const float*)nullptr, partials);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

// ------------------------------------------------------------------ (norm, coefficient) from the partials: one block, fp64, fixed order
//   S = sum of the slots;  norm = gscale * sqrt(S);  coef = gscale if norm < max_norm (optax's trigger, strict) else gscale * max_norm / norm
// No special case for a zero or non-finite norm: IEEE arithmetic gives what optax's where(trigger, t, t / g_norm * max_norm) gives
// (0 -> first branch, inf -> 0, NaN -> NaN).  Thread i adds slots i, i + 256, ...; then a binary tree over the 256 sums.
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, long count, float gscale, double max_norm,
                                                        float* __restrict__ out2) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < count; i += 256) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double gs = (double)gscale;
    const double norm = gs * sqrt(red[0]);
    const double coef = norm < max_norm ? gs : gs * max_norm / norm;
    out2[0] = (float)norm;
    out2[1] = (float)coef;
  }
}
extern "C" int mic_clip_coef(const float* partials, int64_t count, float grad_scale, double max_norm, float* out2, void* stream) {
  MIC_CHECK(partials && out2 && count > 0, "mic_clip_coef: bad args (count must be positive)");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)count, grad_scale, max_norm, out2);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
