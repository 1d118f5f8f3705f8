// adamw_update.inc — THE AdamW element update, included as the body of adamw_kernel, adamw_acc_kernel and adamw_clip_kernel
// (optimizer.hip).  Not a stand-alone header: it expects in scope
//   ROWS, ACC                                      constant expressions
//   n, p, m, v, g, acc, p_lp, lr, t, gscale, b1, b2, omb1, omb2, eps, wd, row_flag, row_f4, want
// (acc is read only with ACC; row_flag, row_f4 and want only with ROWS).
// An include, not a function and not one wider template:
//   * as a __device__ __forceinline__ function called from the three kernels, every kernel's instruction schedule changes, and with
//     such a library the small fp8 training runs became bimodal (profiles/NOTES_r8.md §2, still open);
//   * as one __global__ template adamw_kernel<ROWS, ACC, DEV> the vector instructions stay but every kernel name changes, and the
//     names adamw_kernel<false> / <true> are what the committed product profiles and tests/util_rowop_cases.py know.
//   Included as text, adamw_kernel and adamw_acc_kernel compile to the instructions they had as separate copies (profiles/NOTES_r11.md).
// tests/util_rowop_ref.py (adamw_ref, adamw_consts) restates the operation order below; the two change together.
  const float bc1 = 1.0f - powf(b1, t), bc2 = 1.0f - powf(b2, t);
  const long n4 = n >> 2;
  // ROWS: a block walks whole rows (one flag test per row and block, uniform), its threads the row's float4s
  const long outer_n = ROWS ? n4 / row_f4 : n4;
  const long outer_0 = ROWS ? blockIdx.x : (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long outer_step = ROWS ? gridDim.x : (long)gridDim.x * blockDim.x;
  for (long o = outer_0; o < outer_n; o += outer_step) {
    if constexpr (ROWS) {
      if ((row_flag[o] != 0) != (want != 0)) continue;
    }
    for (long e = ROWS ? o * row_f4 + threadIdx.x : o; e < (ROWS ? (o + 1) * row_f4 : o + 1); e += ROWS ? blockDim.x : 1) {
      float4 pp = reinterpret_cast<float4*>(p)[e], mm = reinterpret_cast<float4*>(m)[e], vv = reinterpret_cast<float4*>(v)[e];
      float4 gg = reinterpret_cast<const float4*>(g)[e];
      if constexpr (ACC) {  // g' = fp32(g + acc): the sum is rounded on its own, before the scale
        const float4 aa = reinterpret_cast<const float4*>(acc)[e];
        gg = make_float4(__fadd_rn(gg.x, aa.x), __fadd_rn(gg.y, aa.y), __fadd_rn(gg.z, aa.z), __fadd_rn(gg.w, aa.w));
      }
      float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
      // a plain multiply: the product feeds multiplies only, so nothing can contract into it
      const float ga[4] = {gg.x * gscale, gg.y * gscale, gg.z * gscale, gg.w * gscale};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
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
