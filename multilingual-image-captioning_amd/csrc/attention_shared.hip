// attention_shared.hip — one-tile cross-attention with K / V shared by G query sequences (mic_attn_fwd_shared / mic_attn_bwd_shared): a unit
// of its own beside attention.hip, built from the same tile text (attention_tile.h)
#include "common.h"
#include <type_traits>
#include "attention_tile.h"

// ------------------------------------------------------------------ cross-attention with K / V shared by G query sequences
// Training on several captions per image: the B = n_img * G query sequences are image-major, sequence b attends the Tk dense key /
// value rows of image b / G.  No key mask, no causal flag (cross-attention has neither); one 64x64 tile per sequence.
// Forward: attn_fwd_kernel's arithmetic, one workgroup per (caption, head) — only the k / v row base differs, so out and lse are bit
// for bit those of the one-tile kernels on K / V rows replicated G times.
template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_shared_kernel(int G, int H, int Tq_max, int Tk, const T* __restrict__ q, int ldq,
                                                              const T* __restrict__ k, int ldk, const T* __restrict__ v, int ldv,
                                                              T* __restrict__ out, int ldo, float* __restrict__ lse_out, PackedRows pk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TB = Tile<T>::BYTES;
  char* Qt = smem;
  char* Kt = smem + TB;
  char* Vt = smem + 2 * TB;
  char* Pt = smem + 3 * TB;
  float* pmax = reinterpret_cast<float*>(smem + 4 * TB);  // [2 jb][64 queries]
  float* psum = pmax + 128;                               // [2 jb][64 queries]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  int Tq = Tq_max;
  size_t q0 = (size_t)b * Tq_max;
  const size_t k0 = (size_t)(b / G) * Tk;
  if (pk.q_off) { q0 = pk.q_off[b]; Tq = pk.q_len[b]; }
  Tile<T>::template stage<256>(Qt, q + q0 * ldq + h * 64, ldq, Tq, tid);
  Tile<T>::template stage<256>(Kt, k + k0 * ldk + h * 64, ldk, Tk, tid);
  Tile<T>::template stage<256>(Vt, v + k0 * ldv + h * 64, ldv, Tk, tid);
  __syncthreads();
  const int nib = (Tq + 31) >> 5, njb = (Tk + 31) >> 5;
  const int ib = wave >> 1, jb = wave & 1;
  const int i = ib * 32 + (lane & 31);
  f32x16 s;
  zero16(s);
  const bool live = ib < nib && jb < njb;
  if (live) Tile<T>::template mma<false, false>(s, Kt, jb * 32, Qt, ib * 32, lane);
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = jb * 32 + acc_row(r, lane);
    const bool ok = live && j < Tk;
    const float x = ok ? s[r] * SCALE : -INFINITY;
    s[r] = x;
    m = fmaxf(m, x);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (lane < 32) pmax[jb * 64 + i] = m;
  __syncthreads();
  const float mrow = fmaxf(pmax[i], pmax[64 + i]);
  const float m_safe = mrow == -INFINITY ? 0.f : mrow;  // (a query block behind Tq: p = 0, not NaN)
  float l = 0.f;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    float pv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = __expf(s[g4 * 4 + e] - m_safe);
      pv[e] = p;
      l += p;
    }
    Tile<T>::store4(Pt, i, jb * 32 + 8 * g4 + 4 * (lane >> 5), pv);
  }
  l += __shfl_xor(l, 32, 64);
  if (lane < 32) psum[jb * 64 + i] = l;
  __syncthreads();
  if (jb == 0 && lane < 32 && i < Tq && lse_out) lse_out[((size_t)b * H + h) * Tq_max + i] = mrow + logf(psum[i] + psum[64 + i]);
  {
    const int db = wave & 1;  // output block (ib, db)
    if (ib < nib) {
      f32x16 o;
      zero16(o);
      Tile<T>::template mma<false, true>(o, Pt, ib * 32, Vt, db * 32, lane);
      const int d = db * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = ib * 32 + acc_row(r, lane);
        const float lq = psum[qi] + psum[64 + qi];
        if (qi < Tq) ElemT<T>::st(out + (q0 + qi) * ldo + h * 64 + d, lq > 0.f ? o[r] / lq : 0.f);
      }
    }
  }
}

// Backward: one workgroup per (image, head).  K and V are staged once; the workgroup walks the image's G captions in ascending order,
// and per caption stages Q / dO / lse / delta, forms the P and dS tiles and writes dQ exactly as attn_bwd_kernel does (dQ bit for bit
// the one-tile kernels' on replicated K / V).  Wave w keeps its 32x32 blocks of dK = sum_g dS_g^T Q_g and dV = sum_g P_g^T dO_g in
// accumulators across the whole walk and stores them once behind the last caption: one rounding in bf16, no atomics, no scratch
// matrix, a fixed summation order.  Six tiles (V stays live over the walk, so P has a tile of its own) + 512 B of lse / delta.
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_shared_kernel(int G, int H, int Tq_max, int Tk, const T* __restrict__ q, int ldq,
                                                              const T* __restrict__ k, int ldk, const T* __restrict__ v, int ldv,
                                                              const T* __restrict__ out, int ldo, const T* __restrict__ dout, int lddo,
                                                              const float* __restrict__ lse_in, T* __restrict__ dq, int lddq,
                                                              T* __restrict__ dk, int lddk, T* __restrict__ dv, int lddv, PackedRows pk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TB = Tile<T>::BYTES;
  char* Qt = smem;
  char* Kt = smem + TB;
  char* Vt = smem + 2 * TB;
  char* dOt = smem + 3 * TB;
  char* Pt = smem + 4 * TB;
  char* dSt = smem + 5 * TB;
  float* lse_s = reinterpret_cast<float*>(smem + 6 * TB);
  float* delta_s = lse_s + 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int img = blockIdx.x / H, h = blockIdx.x % H;
  const size_t k0 = (size_t)img * Tk;
  Tile<T>::template stage<256>(Kt, k + k0 * ldk + h * 64, ldk, Tk, tid);
  Tile<T>::template stage<256>(Vt, v + k0 * ldv + h * 64, ldv, Tk, tid);
  const int njb = (Tk + 31) >> 5;
  const int xb = wave >> 1, db = wave & 1;
  const int d = db * 32 + (lane & 31);
  f32x16 acc_k, acc_v;
  zero16(acc_k); zero16(acc_v);
  for (int g = 0; g < G; ++g) {
    const int b = img * G + g;
    int Tq = Tq_max;
    size_t q0 = (size_t)b * Tq_max;
    if (pk.q_off) { q0 = pk.q_off[b]; Tq = pk.q_len[b]; }
    if (g) __syncthreads();  // the previous caption's dQ / dK / dV contractions have read Q, dO, P and dS
    Tile<T>::template stage<256>(Qt, q + q0 * ldq + h * 64, ldq, Tq, tid);
    Tile<T>::template stage<256>(dOt, dout + q0 * lddo + h * 64, lddo, Tq, tid);
    {
      // delta_i = dO_i . O_i : thread t covers 16 of the 64 dims of row t>>2
      const int row = tid >> 2, part = tid & 3;
      float dl = 0.f;
      if (row < Tq) {
        const T* orow = out + (q0 + row) * ldo + h * 64 + part * 16;
        const T* drow = dout + (q0 + row) * lddo + h * 64 + part * 16;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float a[8], gg[8];
          ld8(orow + c * 8, a);
          ld8(drow + c * 8, gg);
#pragma unroll
          for (int e = 0; e < 8; ++e) dl += a[e] * gg[e];
        }
      }
      dl += __shfl_xor(dl, 1, 64);
      dl += __shfl_xor(dl, 2, 64);
      if (part == 0) delta_s[row] = dl;
      if (tid < 64) lse_s[tid] = tid < Tq ? lse_in[((size_t)b * H + h) * Tq_max + tid] : 0.f;
    }
    __syncthreads();
    const int nib = (Tq + 31) >> 5;
    {
      // P and dS tiles (rows = queries); rows >= Tq and keys >= Tk are exact zeros
      const int ib = wave >> 1, jb = wave & 1;
      const int i = ib * 32 + (lane & 31);
      const float lse_i = lse_s[i], delta_i = delta_s[i];
      f32x16 sacc, dp;
      zero16(sacc); zero16(dp);
      const bool live = ib < nib && jb < njb;
      if (live) {
        Tile<T>::template mma<false, false>(sacc, Kt, jb * 32, Qt, ib * 32, lane);
        Tile<T>::template mma<false, false>(dp, Vt, jb * 32, dOt, ib * 32, lane);
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float pv[4], dsv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = g4 * 4 + e;
          const int j = jb * 32 + acc_row(r, lane);
          const bool ok = live && i < Tq && j < Tk;
          const float p = ok ? __expf(sacc[r] * SCALE - lse_i) : 0.f;
          pv[e] = p;
          dsv[e] = p * (dp[r] - delta_i) * SCALE;
        }
        Tile<T>::store4(Pt, i, jb * 32 + 8 * g4 + 4 * (lane >> 5), pv);
        Tile<T>::store4(dSt, i, jb * 32 + 8 * g4 + 4 * (lane >> 5), dsv);
      }
    }
    __syncthreads();
    if (xb < nib) {
      f32x16 a;
      zero16(a);
      Tile<T>::template mma<false, true>(a, dSt, xb * 32, Kt, db * 32, lane);  // dQ = dS K
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = xb * 32 + acc_row(r, lane);
        if (i < Tq) ElemT<T>::st(dq + (q0 + i) * lddq + h * 64 + d, a[r]);
      }
    }
    if (xb < njb) {
      Tile<T>::template mma<true, true>(acc_k, dSt, xb * 32, Qt, db * 32, lane);   // dK += dS^T Q
      Tile<T>::template mma<true, true>(acc_v, Pt, xb * 32, dOt, db * 32, lane);   // dV += P^T dO
    }
  }
  if (xb < njb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = xb * 32 + acc_row(r, lane);
      if (j < Tk) {
        ElemT<T>::st(dk + (k0 + j) * lddk + h * 64 + d, acc_k[r]);
        ElemT<T>::st(dv + (k0 + j) * lddv + h * 64 + d, acc_v[r]);
      }
    }
  }
}

// ------------------------------------------------------------------ host side
struct SharedCall { int dtype, n_img, G, H, Tq, Tk; const int32_t* q_off; const int32_t* q_len; int ldq, ldk, ldv, ldo, lddo; };

// the limits of both entry points (a refused call launches nothing): one 64x64 tile per sequence, the dtypes of the one-tile cores, and
// the row-stride alignment of mic_attn_fwd_packed (16-B staging loads of q / k / v and, backward, of out / dout)
static int shared_check(const char* fn, const SharedCall& c, bool ptrs_ok, bool bwd) {
  MIC_CHECK(c.n_img > 0 && c.G >= 1 && c.H > 0 && c.Tq > 0 && c.Tk > 0, "%s: bad shape n_img=%d G=%d H=%d Tq_max=%d Tk=%d", fn, c.n_img, c.G, c.H, c.Tq, c.Tk);
  MIC_CHECK(c.Tq <= 64 && c.Tk <= 64, "%s: one 64x64 tile per sequence (Tq_max=%d Tk=%d)", fn, c.Tq, c.Tk);
  MIC_CHECK((long long)c.n_img * c.G * c.H <= 0x7fffffffLL, "%s: too many workgroups (n_img=%d G=%d H=%d)", fn, c.n_img, c.G, c.H);
  MIC_CHECK(ptrs_ok && (!c.q_off == !c.q_len), "%s: null pointer (q_off and q_len go together)", fn);
  MIC_CHECK(c.dtype == MIC_BF16 || c.dtype == MIC_F32, "%s: bad dtype", fn);
  const int align = c.dtype == MIC_BF16 ? 8 : 4;
  MIC_CHECK(c.ldq % align == 0 && c.ldk % align == 0 && c.ldv % align == 0 && (!bwd || (c.ldo % align == 0 && c.lddo % align == 0)),
            "%s: row strides must keep 16-B alignment", fn);
  return MIC_OK;
}

template <typename K>
static int shared_set_lds(K kernel, size_t bytes) {
  if (bytes > 65536) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { mic_set_error("hipFuncSetAttribute(%zu): %s", bytes, hipGetErrorString(e)); return MIC_ELAUNCH; }
  }
  return MIC_OK;
}

template <typename T>
static int launch_fwd_shared(const SharedCall& c, const void* q, const void* k, const void* v, void* out, float* lse, void* stream) {
  const size_t lds = 4 * Tile<T>::BYTES + 1024;
  if (int rc = shared_set_lds(attn_fwd_shared_kernel<T>, lds)) return rc;
  hipLaunchKernelGGL(attn_fwd_shared_kernel<T>, dim3(c.n_img * c.G * c.H), dim3(256), lds, (hipStream_t)stream, c.G, c.H, c.Tq, c.Tk, (const T*)q, c.ldq,
                     (const T*)k, c.ldk, (const T*)v, c.ldv, (T*)out, c.ldo, lse, PackedRows{c.q_off, c.q_len, 0});
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
template <typename T>
static int launch_bwd_shared(const SharedCall& c, const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                             void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, void* stream) {
  const size_t lds = 6 * Tile<T>::BYTES + 512;
  if (int rc = shared_set_lds(attn_bwd_shared_kernel<T>, lds)) return rc;
  hipLaunchKernelGGL(attn_bwd_shared_kernel<T>, dim3(c.n_img * c.H), dim3(256), lds, (hipStream_t)stream, c.G, c.H, c.Tq, c.Tk, (const T*)q, c.ldq,
                     (const T*)k, c.ldk, (const T*)v, c.ldv, (const T*)out, c.ldo, (const T*)dout, c.lddo, lse, (T*)dq, lddq, (T*)dk, lddk, (T*)dv, lddv,
                     PackedRows{c.q_off, c.q_len, 0});
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}

extern "C" int mic_attn_fwd_shared(int dtype, int n_img, int G, int H, int Tq_max, int Tk, const int32_t* q_off, const int32_t* q_len,
                                   const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, float* lse,
                                   void* stream) {
  const SharedCall c{dtype, n_img, G, H, Tq_max, Tk, q_off, q_len, ldq, ldk, ldv, ldo, 0};
  if (int rc = shared_check("mic_attn_fwd_shared", c, q && k && v && out, false)) return rc;
  return dtype == MIC_BF16 ? launch_fwd_shared<uint16_t>(c, q, k, v, out, lse, stream) : launch_fwd_shared<float>(c, q, k, v, out, lse, stream);
}
extern "C" int mic_attn_bwd_shared(int dtype, int n_img, int G, int H, int Tq_max, int Tk, const int32_t* q_off, const int32_t* q_len,
                                   const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* out, int ldo,
                                   const void* dout, int lddo, const float* lse, void* dq, int lddq, void* dk, int lddk, void* dv, int lddv,
                                   void* stream) {
  const SharedCall c{dtype, n_img, G, H, Tq_max, Tk, q_off, q_len, ldq, ldk, ldv, ldo, lddo};
  if (int rc = shared_check("mic_attn_bwd_shared", c, q && k && v && out && dout && lse && dq && dk && dv, true)) return rc;
  return dtype == MIC_BF16 ? launch_bwd_shared<uint16_t>(c, q, k, v, out, dout, lse, dq, lddq, dk, lddk, dv, lddv, stream)
                           : launch_bwd_shared<float>(c, q, k, v, out, dout, lse, dq, lddq, dk, lddk, dv, lddv, stream);
}
