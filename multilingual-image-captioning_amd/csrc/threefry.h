// threefry.h — the threefry2x32 block function of jax 0.2.16's PRNG and the Gumbel noise of jax.random.categorical built on it [restated from the published algorithm; pinned on the Random123 / JAX
// known-answer vectors in tests/test_oracle_cpu.py], shared by the sampling kernels of decode.hip and sample_keyed.hip.
#pragma once
#include <stdint.h>

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  const int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += ks[0]; x1 += ks[1];
#pragma unroll
  for (int g = 0; g < 5; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { x0 += x1; x1 = rotl32(x1, R[g & 1][i]); x1 ^= x0; }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
}

// Gumbel noise of element e of an n-element array drawn with key (k0, k1), as jax.random.gumbel makes it: the counter array (padded to
// even) is split in halves x0 | x1 at h = (n + 1) / 2, element e < h uses word 0 of the block (e, e + h), element e >= h word 1 of
// (e - h, e); uniform = max(tiny, (bitcast(bits >> 9 | 0x3f800000) - 1) * (1 - tiny) + tiny); gumbel = -log(-log(uniform)).
__device__ __forceinline__ float gumbel_noise(uint32_t k0, uint32_t k1, uint32_t e, uint32_t h, uint32_t n) {
  uint32_t c0, c1;
  if (e < h) { c0 = e; c1 = e + h < n ? e + h : 0u; } else { c0 = e - h; c1 = e; }
  threefry2x32(k0, k1, c0, c1);
  const uint32_t bits = e < h ? c0 : c1;
  const float f = __uint_as_float((bits >> 9) | 0x3f800000u) - 1.0f;
  const float tiny = 1.17549435e-38f;
  const float u = fmaxf(tiny, f * (1.0f - tiny) + tiny);
  return -logf(-logf(u));
}
