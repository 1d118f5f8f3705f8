// score_rows.hip — the row kernels behind model.score: cross-entropy rows from the head GEMM's softmax partials with the label's logit
// read from a vector (mic_ce_rows_picked: the head launch gemm_d2_kernel<2> stored no logits and left it there), and per-caption sums
// of the token terms (mic_segment_sums).  A unit of its own beside elementwise.hip, with which it shares the merge of the partials
// (ce_tiles_merge.h); its resource table is tests/golden/kernel_resources_units_score.json.
#include "ce_tiles_merge.h"

// ce_rows_tiles_kernel (elementwise.hip) with the label's logit from a vector (the head launch that stored no logits left it there: mic_gemm_args.pick_out)
__global__ __launch_bounds__(256) void picked_nll_rows_kernel(int rows, const float2* __restrict__ stat, int stat_ld, int ntiles,
                                                            const float* __restrict__ label_logit, float* __restrict__ row_lse,
                                                            float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float lse = ce_tiles_lse(stat, stat_ld, ntiles, row, lane);
  if (lane == 0) {
    row_lse[row] = lse;
    row_loss[row] = lse - label_logit[row];
  }
}
extern "C" int mic_ce_rows_picked(int rows, int V, const float* rowstat, int stat_ld, const float* label_logit, float* row_lse, float* row_loss,
                                  void* stream) {
  const int ntiles = (V + 63) / 64;
  MIC_CHECK(rows > 0 && V > 1 && rowstat && label_logit && row_lse && row_loss && stat_ld >= ntiles && ((uintptr_t)rowstat & 7) == 0, "mic_ce_rows_picked: bad args");
  hipLaunchKernelGGL(picked_nll_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, (const float2*)rowstat, stat_ld, ntiles, label_logit, row_lse, row_loss);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
// out[s] = scale * sum of x over segment s: one wave per segment; lane l adds elements l, l + 64, ... in order, wave_sum's fixed tree
// joins the lanes — the order is a function of seg_len[s] alone, whatever the grid
__global__ __launch_bounds__(256) void segment_sums_kernel(int n_seg, const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_len,
                                                          const float* __restrict__ x, float scale, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_seg) return;
  const int n = seg_len[sg];
  const float* xs = x + (size_t)seg_off[sg];
  float a = 0.f;
  for (int i = lane; i < n; i += 64) a += xs[i];
  a = wave_sum(a);
  if (lane == 0) out[sg] = n > 0 ? scale * a : 0.f;
}
extern "C" int mic_segment_sums(int n_seg, const int32_t* seg_off, const int32_t* seg_len, const float* x, float scale, float* out, void* stream) {
  MIC_CHECK(n_seg > 0 && seg_off && seg_len && x && out, "mic_segment_sums: bad args");
  hipLaunchKernelGGL(segment_sums_kernel, dim3((n_seg + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_seg, seg_off, seg_len, x, scale, out);
  MIC_LAUNCH_CHECK();
  return MIC_OK;
}
