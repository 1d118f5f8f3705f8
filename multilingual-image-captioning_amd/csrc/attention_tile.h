// attention_tile.h — the 64x64 LDS tiles of the attention cores and their helpers (moved as text out of attention.hip, which
// includes it; attention_shared.hip builds its kernels from the same text)
#pragma once
#include "common.h"
#include <type_traits>

#define SCALE 0.125f  // 1/sqrt(64): q is scaled before q.k^T (power of two: exact either side of the product)

// ------------------------------------------------------------------ 64x64 LDS tiles
template <typename T> struct Tile;

template <> struct Tile<uint16_t> {
  static constexpr int BYTES = 64 * 64 * 2;
  // 16-B chunk index XOR-swizzled by row.  The same tile is read two ways: ds_read_b128 along k (lane <-> row: the 16-lane
  // groups {0-3,12-15,20-27}/... cover 8 distinct row PAIRS, so any bijection of the pair index p = (row>>1)&7 is conflict-
  // free) and ds_read_b64_tr_b16 across 4 consecutive rows x 4 chunks (rows k0,k0+1 vs k0+2,k0+3 must land in different
  // aligned blocks of 4 chunks: bit 2 of the swizzle = bit 0 of p).  sw(row) = ((p & 1) << 2) | (p >> 1) satisfies both;
  // row & 7 (the first version) measured 28 % / 42 % of LDS cycles as bank conflicts in the fwd / bwd kernels.
  static __device__ __forceinline__ int sw(int row) { const int p = (row >> 1) & 7; return ((p & 1) << 2) | (p >> 1); }
  // element (row, col) -> byte offset
  static __device__ __forceinline__ int off(int row, int col) { return row * 128 + ((((col >> 3) ^ sw(row)) << 4) | ((col & 7) << 1)); }
  // stage rows [0,nrows) x 64 cols from src (row stride ld); rows >= nrows are zero
  template <int NT = 64>
  static __device__ __forceinline__ void stage(char* t, const uint16_t* src, int ld, int nrows, int lane) {
#pragma unroll
    for (int it = 0; it < 512 / NT; ++it) {
      const int idx = it * NT + lane, row = idx >> 3, c = idx & 7;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < nrows) v = *reinterpret_cast<const uint4*>(src + (size_t)row * ld + c * 8);
      *reinterpret_cast<uint4*>(t + row * 128 + ((c ^ sw(row)) << 4)) = v;
    }
  }
  template <bool KM>
  static __device__ __forceinline__ bf16x8 frag(const char* t, int xb, int kk, int lane) {
    if (!KM) {
      const int row = xb + (lane & 31), kc = kk * 2 + (lane >> 5);
      return *reinterpret_cast<const bf16x8*>(t + row * 128 + ((kc ^ sw(row)) << 4));
    } else {
      const int g = lane >> 4, p = lane & 15;
      const int x = xb + 16 * (g & 1) + (p & 3) * 4;
      const int k = kk * 16 + 8 * (g >> 1) + (p >> 2);
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, t + off(k, x)));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, t + off(k + 4, x)));
      s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      return __builtin_bit_cast(bf16x8, r);
    }
  }
  // acc(32x32) += sum_k A(a0+i, k) * B(k, b0+j) over k in [0,64).  AKM: A tile stored [k][i]; BKM: B tile stored [k][j]
  // (non-KM B tile is stored [j][k]).
  template <bool AKM, bool BKM>
  static __device__ __forceinline__ void mma(f32x16& acc, const char* At, int a0, const char* Bt, int b0, int lane) {
    // the four k-steps accumulate into ONE block: all fragment reads go out first, pinned in front of the MFMAs (the scheduler
    // otherwise sinks each pair of reads next to its MFMA and waits an LDS round trip per k-step)
    bf16x8 a[4], b[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      a[kk] = frag<AKM>(At, a0, kk, lane);
      b[kk] = frag<BKM>(Bt, b0, kk, lane);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kk], b[kk], acc, 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, ((AKM ? 2 : 1) + (BKM ? 2 : 1)) * 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
  }
  static __device__ __forceinline__ void store4(char* t, int row, int col0, const float* v) {
    uint2 o;
    o.x = f2bf_pk(v[0], v[1]);
    o.y = f2bf_pk(v[2], v[3]);
    *reinterpret_cast<uint2*>(t + off(row, col0)) = o;
  }
};

template <> struct Tile<float> {
  static constexpr int BYTES = 64 * 64 * 4;
  template <int NT = 64>
  static __device__ __forceinline__ void stage(char* t, const float* src, int ld, int nrows, int lane) {
    float* f = reinterpret_cast<float*>(t);
#pragma unroll
    for (int it = 0; it < 1024 / NT; ++it) {
      const int idx = it * NT + lane, row = idx >> 4, c = idx & 15;
      float4 v = make_float4(0, 0, 0, 0);
      if (row < nrows) v = *reinterpret_cast<const float4*>(src + (size_t)row * ld + c * 4);
      *reinterpret_cast<float4*>(f + row * 64 + c * 4) = v;
    }
  }
  template <bool AKM, bool BKM>
  static __device__ __forceinline__ void mma(f32x16& acc, const char* At, int a0, const char* Bt, int b0, int lane) {
    const float* A = reinterpret_cast<const float*>(At);
    const float* B = reinterpret_cast<const float*>(Bt);
    const int i = lane & 31, h = lane >> 5;
#pragma unroll 8
    for (int s = 0; s < 32; ++s) {
      const int k = 2 * s + h;
      const float a = AKM ? A[k * 64 + a0 + i] : A[(a0 + i) * 64 + k];
      const float b = BKM ? B[k * 64 + b0 + i] : B[(b0 + i) * 64 + k];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  static __device__ __forceinline__ void store4(char* t, int row, int col0, const float* v) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(t) + row * 64 + col0) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
// accumulator element r of a 32x32 block: row (r&3) + 8*(r>>2) + 4*(lane>>5), col lane&31
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Variable-length ("packed") rows: sequence b owns the q rows [q_off[b], q_off[b] + q_len[b]) of a packed [sum q_len][ld] matrix
// (no rows for padded positions at all).  kv_packed: keys / values are the same packed rows (self-attention) — otherwise every
// sequence has its Tk dense rows [b*Tk, (b+1)*Tk) (cross-attention over the encoder states).  q_off == nullptr: dense rows.
struct PackedRows { const int32_t* q_off; const int32_t* q_len; int kv_packed; };
