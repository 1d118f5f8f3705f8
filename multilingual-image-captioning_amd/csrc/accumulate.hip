// accumulate.hip — gradient accumulation (N micro-batches per AdamW step): the running fp32 sum beside the optimizer and AdamW on
// g + acc.  A unit of its own: elementwise.hip and its AdamW kernels stay text for text (and instruction for instruction) what they
// were, and this unit's compiler listing goes with its own table (tests/golden/kernel_resources_accumulate.json, see the Makefile).
#include "common.h"

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

// AdamW on g' = fp32(g + acc): the final micro-step of an accumulation reads the running sum itself instead of a separate
// 12 B/element pass in front of the update.  The sum is rounded to fp32 BEFORE gscale is applied (__fadd_rn / __fmul_rn: no
// contraction across the two), so the result is bit for bit adamw_kernel's (elementwise.hip) on a pre-summed gradient.
template <bool ROWS>
__global__ __launch_bounds__(256) void adamw_acc_kernel(long n, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, const float* __restrict__ acc,
                                                        uint16_t* __restrict__ p_lp, const float* __restrict__ hyper, float b1, float b2,
                                                        float omb1, float omb2, float eps, float wd, float gscale,
                                                        const uint8_t* __restrict__ row_flag, int row_f4, int want) {
  const float lr = hyper[0], t = hyper[1];
  const float bc1 = 1.0f - powf(b1, t), bc2 = 1.0f - powf(b2, t);
  const long n4 = n >> 2;
  const long outer_n = ROWS ? n4 / row_f4 : n4;
  const long outer_0 = ROWS ? blockIdx.x : (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long outer_step = ROWS ? gridDim.x : (long)gridDim.x * blockDim.x;
  for (long o = outer_0; o < outer_n; o += outer_step) {
    if constexpr (ROWS) {
      if ((row_flag[o] != 0) != (want != 0)) continue;
    }
    for (long e = ROWS ? o * row_f4 + threadIdx.x : o; e < (ROWS ? (o + 1) * row_f4 : o + 1); e += ROWS ? blockDim.x : 1) {
      float4 pp = reinterpret_cast<float4*>(p)[e], mm = reinterpret_cast<float4*>(m)[e], vv = reinterpret_cast<float4*>(v)[e];
      const float4 gg = reinterpret_cast<const float4*>(g)[e], aa = reinterpret_cast<const float4*>(acc)[e];
      float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
      const float ga[4] = {__fmul_rn(__fadd_rn(gg.x, aa.x), gscale), __fmul_rn(__fadd_rn(gg.y, aa.y), gscale),
                           __fmul_rn(__fadd_rn(gg.z, aa.z), gscale), __fmul_rn(__fadd_rn(gg.w, aa.w), gscale)};
  #pragma unroll
      for (int i = 0; i < 4; ++i) {  // adamw_kernel's update, statement for statement
        ma[i] = b1 * ma[i] + omb1 * ga[i];
        va[i] = b2 * va[i] + omb2 * ga[i] * ga[i];
        const float upd = (ma[i] / bc1) / (sqrtf(va[i] / bc2) + eps) + wd * pa[i];
        pa[i] -= lr * upd;
      }
      reinterpret_cast<float4*>(p)[e] = make_float4(pa[0], pa[1], pa[2], pa[3]);
      reinterpret_cast<float4*>(m)[e] = make_float4(ma[0], ma[1], ma[2], ma[3]);
      reinterpret_cast<float4*>(v)[e] = make_float4(va[0], va[1], va[2], va[3]);
      if (p_lp) {
        uint2 q;
        q.x = f2bf_pk(pa[0], pa[1]);
        q.y = f2bf_pk(pa[2], pa[3]);
        reinterpret_cast<uint2*>(p_lp)[e] = q;
      }
    }
  }
}
extern "C" int mic_adamw_acc(int64_t n, float* p, float* m, float* v, const float* g, const float* acc, void* p_lp, const float* hyper,
                             double b1, double b2, double eps, double wd, float grad_scale, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && p && m && v && g && acc && hyper, "mic_adamw_acc: bad args (n must be a multiple of 4)");
  long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(adamw_acc_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, acc, (uint16_t*)p_lp, hyper,
                     (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd, grad_scale, (const uint8_t*)nullptr, 1, 0);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
extern "C" int mic_adamw_rows_acc(int64_t rows, int width, const uint8_t* row_flag, int want, float* p, float* m, float* v, const float* g,
                                  const float* acc, void* p_lp, const float* hyper, double b1, double b2, double eps, double wd,
                                  float grad_scale, void* stream) {
  MIC_CHECK(rows > 0 && width > 0 && width % 4 == 0 && row_flag && p && m && v && g && acc && hyper,
            "mic_adamw_rows_acc: bad args (width must be a multiple of 4)");
  const long n = (long)rows * width;
  long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(adamw_acc_kernel<true>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, n, p, m, v, g, acc, (uint16_t*)p_lp, hyper,
                     (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd, grad_scale, row_flag, width / 4, want);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
