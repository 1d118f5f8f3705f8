// clip.hip — global-norm gradient clipping (optax.clip_by_global_norm in front of AdamW): a sum of squares with a fixed summation
// order, the kernel that turns it into (norm, coefficient), and AdamW with its gradient scale read from device memory, so the host
// never waits for the norm.  A unit of its own, like accumulate.hip: elementwise.hip and accumulate.hip stay text for text what they
// were, and this unit's compiler listing goes with its own table (tests/golden/kernel_resources_clip.json, see the Makefile).
#include "common.h"

#define SUMSQ_MAX_BLOCKS 1024  // ~4 blocks per CU: one slot per block, so a step of a few dozen buckets leaves tens of thousands of slots
#define ALIGNED16(p) ((reinterpret_cast<uintptr_t>(p) & 15) == 0)

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

// ------------------------------------------------------------------ AdamW with the gradient scale read from device memory
// adamw_kernel (elementwise.hip) / adamw_acc_kernel (accumulate.hip) with gscale = *coef: the scaled gradient is rounded on its own
// (__fmul_rn, after __fadd_rn with ACC), so p, m, v and p_lp are bit for bit those of mic_adamw / mic_adamw_acc called with that float.
template <bool ACC>
__global__ __launch_bounds__(256) void adamw_clip_kernel(long n, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ g, const float* __restrict__ acc,
                                                         uint16_t* __restrict__ p_lp, const float* __restrict__ hyper,
                                                         const float* __restrict__ coef, float b1, float b2, float omb1, float omb2,
                                                         float eps, float wd) {
  const float lr = hyper[0], t = hyper[1], gscale = coef[0];
  const float bc1 = 1.0f - powf(b1, t), bc2 = 1.0f - powf(b2, t);
  const long n4 = n >> 2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[e], mm = reinterpret_cast<float4*>(m)[e], vv = reinterpret_cast<float4*>(v)[e];
    float4 gg = reinterpret_cast<const float4*>(g)[e];
    if constexpr (ACC) {
      const float4 aa = reinterpret_cast<const float4*>(acc)[e];
      gg = make_float4(__fadd_rn(gg.x, aa.x), __fadd_rn(gg.y, aa.y), __fadd_rn(gg.z, aa.z), __fadd_rn(gg.w, aa.w));
    }
    float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
    const float ga[4] = {__fmul_rn(gg.x, gscale), __fmul_rn(gg.y, gscale), __fmul_rn(gg.z, gscale), __fmul_rn(gg.w, gscale)};
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
extern "C" int mic_adamw_clip(int64_t n, float* p, float* m, float* v, const float* g, const float* acc, void* p_lp, const float* hyper,
                              const float* coef, double b1, double b2, double eps, double wd, void* stream) {
  MIC_CHECK(n > 0 && n % 4 == 0 && p && m && v && g && hyper && coef, "mic_adamw_clip: bad args (n must be a multiple of 4)");
  MIC_CHECK(ALIGNED16(p) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(g) && ALIGNED16(acc) && (reinterpret_cast<uintptr_t>(p_lp) & 7) == 0,
            "mic_adamw_clip: p, m, v, g and acc must be 16-byte aligned (p_lp: 8-byte)");
  long nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
  if (acc) hipLaunchKernelGGL(adamw_clip_kernel<true>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, acc, (uint16_t*)p_lp,
                              hyper, coef, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd);
  else hipLaunchKernelGGL(adamw_clip_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (long)n, p, m, v, g, (const float*)nullptr,
                          (uint16_t*)p_lp, hyper, coef, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
