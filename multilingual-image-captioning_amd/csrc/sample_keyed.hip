// sample_keyed.hip — several categorical draws per image in one launch (generate(do_sample=True, num_return_sequences=N)), each draw
// with its own key read from device memory, and the log-probability of every draw.  A unit of its own beside decode.hip (whose
// sample_rows_kernel draws its noise from the same device function, gumbel_noise of threefry.h).
#include "common.h"
#include "threefry.h"

__global__ void keyed_fill_i32_kernel(int32_t* p, int n, int v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ keyed sampling: several draws per image (gen:537-663)
// generate(do_sample=True, num_return_sequences=N) runs N independent `_sample` chains (gen:537-663) over the same images as ONE
// chain of R = images * draws rows, row r = image * draws + n.  Draw n is its own call of jax.random.categorical over an
// [images][V] array with its own key: row r takes key keys[n] (read from device memory, so a captured step does not freeze a call's
// keys) and the counters of row `image` of that [images][V] array — element e = image * V + i of n_total = images * V, halves and
// odd-count padding exactly as in sample_rows_kernel (decode.hip).  The arithmetic per entry (division by the temperature, EOS
// suppression, the (thr, tie_limit) mask, lowest index on ties) is that kernel's, the noise the same gumbel_noise (threefry.h): with
// draws == 1 the ids are bit for bit those of mic_sample_rows.  Differences in work, not in results:
//   * an entry that is -inf after suppression and thresholds gets no threefry block and no logf (-inf + noise is -inf): with
//     top_k = 50 that is all but 50 of the 250 054 columns of a row;
//   * the row is read with 16-byte loads between a scalar head (up to the first 16-byte boundary of the row) and tail;
//   * the same pass keeps an online (max, sum-exp) over the surviving entries v (the distribution the draw is made from: the raw
//     logits in the reference's mode, the processed ones otherwise), merged over the block in a fixed order, and one thread adds
//     log p(drawn) = (v[drawn] - max) - logf(sum) to score[row] unless finished[row] is set (both optional).  mic_greedy_step runs
//     after this kernel, so the EOS draw itself still counts; a forced token is a point mass and adds 0.
// (max, sum-exp) += one finite value / another pair; an empty pair is (-inf, 0)
__device__ __forceinline__ void lse_push(float& m, float& s, float v) {
  if (v > m) { s = s * __expf(m - v) + 1.0f; m = v; }
  else s += __expf(v - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mn = fmaxf(m, om);
  if (mn == -INFINITY) return;  // both empty
  s = s * __expf(m - mn) + os * __expf(om - mn);
  m = mn;
}

template <typename T> struct Vec16;  // the elements of one 16-byte load as floats
template <> struct Vec16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4& r, float* f) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  }
};
template <> struct Vec16<uint16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4& r, float* f) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
  }
};

template <typename T>
__global__ __launch_bounds__(1024) void sample_rows_keyed_kernel(int images, int draws, int V, const T* __restrict__ logits, int ld,
                                                                 const uint32_t* __restrict__ keys, float temperature,
                                                                 int suppress_eos, int eos, const float* __restrict__ min_keep,
                                                                 const int32_t* __restrict__ tie_limit, int32_t* __restrict__ out,
                                                                 const int32_t* __restrict__ finished, float* __restrict__ score) {
  const int row = blockIdx.x, image = row / draws, draw = row - image * draws;
  const uint32_t k0 = keys[2 * draw], k1 = keys[2 * draw + 1];
  const uint32_t n = (uint32_t)images * (uint32_t)V, h = (n + 1u) >> 1, e0 = (uint32_t)image * (uint32_t)V;
  const T* x = logits + (size_t)row * ld;
  const float thr = min_keep ? min_keep[row] : -INFINITY;
  const int lim = tie_limit ? tie_limit[row] : 0x7fffffff;
  float best = -INFINITY, bv = -INFINITY;  // best noisy value, and the value v it was formed from
  int bi = 0x7fffffff;
  float m = -INFINITY, s = 0.f;

  auto consider = [&](int i, float v) {
    if (temperature != 1.0f) v = v / temperature;
    if ((suppress_eos && i == eos) || v < thr || (v == thr && i >= lim)) v = -INFINITY;
    float c = v;
    if (v > -INFINITY) {
      c = v + gumbel_noise(k0, k1, e0 + (uint32_t)i, h, n);
      lse_push(m, s, v);
    }
    if (c > best || (c == best && i < bi)) { best = c; bi = i; bv = v; }
  };

  constexpr int VEC = Vec16<T>::N;
  const int tid = threadIdx.x, nthr = blockDim.x;
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) / (unsigned)sizeof(T));
  head = head < V ? head : V;
  const int nvec = (V - head) / VEC, tail = head + nvec * VEC;
  if (tid < head) consider(tid, ElemT<T>::ld(x + tid));
  for (int q = tid; q < nvec; q += nthr) {
    const int i0 = head + q * VEC;
    const uint4 raw = *reinterpret_cast<const uint4*>(x + i0);
    float f[VEC];
    Vec16<T>::unpack(raw, f);
#pragma unroll
    for (int j = 0; j < VEC; ++j) consider(i0 + j, f[j]);
  }
  if (tail + tid < V) consider(tail + tid, ElemT<T>::ld(x + tail + tid));  // fewer than VEC entries

  // argmax: a total order (value, then lower index), so any reduction shape gives the same winner; (max, sum-exp): lane 0's tree
  // of shuffles, then wave 0 .. wave 15 in turn
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_down(best, o, 64), ovv = __shfl_down(bv, o, 64);
    const int oi = __shfl_down(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; bv = ovv; }
    const float om = __shfl_down(m, o, 64), os = __shfl_down(s, o, 64);
    lse_merge(m, s, om, os);
  }
  __shared__ float sv[16], svv[16], sm[16], ss[16];
  __shared__ int si[16];
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) { sv[wave] = best; si[wave] = bi; svv[wave] = bv; sm[wave] = m; ss[wave] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < (nthr >> 6); ++w) {
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; bv = svv[w]; }
      lse_merge(m, s, sm[w], ss[w]);
    }
    out[row] = bi;
    // nothing survived (cannot arise through generate(): the warpers keep a token): index 0 as in sample_rows_kernel, no score
    if (score && !(finished && finished[row]) && bv > -INFINITY) score[row] += (bv - m) - logf(s);
  }
}

extern "C" int mic_sample_rows_keyed(int dtype, int images, int draws, int V, const void* logits, int ld, const uint32_t* keys,
                                     float temperature, int forced_token, int suppress_eos, int eos_token_id,
                                     const float* min_keep, const int32_t* tie_limit, int32_t* out_idx, const int32_t* finished,
                                     float* score, void* stream) {
  MIC_CHECK(images > 0 && draws > 0 && V > 0 && ld >= V && logits && keys && out_idx && temperature > 0.f && forced_token < V,
            "mic_sample_rows_keyed: bad args");
  MIC_CHECK((uint64_t)images * (uint64_t)V < (1ull << 32), "mic_sample_rows_keyed: images*V must fit the 32-bit threefry counter");
  MIC_CHECK((uint64_t)images * (uint64_t)draws < (1ull << 31), "mic_sample_rows_keyed: images*draws rows exceed the grid");
  MIC_CHECK(dtype == MIC_BF16 || dtype == MIC_F32, "mic_sample_rows_keyed: bad dtype");
  MIC_CHECK(reinterpret_cast<uintptr_t>(logits) % (dtype == MIC_BF16 ? 2 : 4) == 0, "mic_sample_rows_keyed: logits not aligned to their element");
  const int R = images * draws;
  if (forced_token >= 0) {  // ForcedBOS / ForcedEOS: a point mass — every row draws that token, log p = 0
    hipLaunchKernelGGL(keyed_fill_i32_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, out_idx, R, forced_token);
    MIC_LAUNCH_CHECK();
    return MIC_OK;
  }
  dim3 grid(R), block(1024);
  if (dtype == MIC_BF16)
    hipLaunchKernelGGL(sample_rows_keyed_kernel<uint16_t>, grid, block, 0, (hipStream_t)stream, images, draws, V, (const uint16_t*)logits, ld, keys, temperature, suppress_eos, eos_token_id, min_keep, tie_limit, out_idx, finished, score);
  else
    hipLaunchKernelGGL(sample_rows_keyed_kernel<float>, grid, block, 0, (hipStream_t)stream, images, draws, V, (const float*)logits, ld, keys, temperature, suppress_eos, eos_token_id, min_keep, tie_limit, out_idx, finished, score);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
