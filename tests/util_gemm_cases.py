"""The case table of the GEMM conformance suite, shared by tests/test_gemm_conformance_gpu.py (which runs every case) and
tests/test_gemm_conformance_cpu.py (which asserts, on the host planner alone, that each case still gets the plan it claims —
so a planner change that moves a case off its kernel fails a test instead of shrinking the coverage silently).

A case: shape (M, N, K), operand layout (akm = a_kmajor, bkm = b_kmajor), dtype ("bf16" / "e4m3" / "e5m2": fp8 with A in
that format, B e4m3), the CU budget (0 = default), the epilogue features, the plan it targets and the kernel that plan
launches (asserted against the name mic_gemm_plan's report spells, kernel_name below, and against the committed coverage profile).  `group`: a grouped launch, one feature
dict per problem.

Features: alpha, bias, act, zout, dact, drop (p), res, acc, c32 (fp32 C), split (split_k), slabs (split-K into fp32 slabs +
mic_sum_slabs), rowsum (a_rowsum), rowsum_k, k_valid, rowstat, nvalid, ln (folded LayerNorm), rowsum2, ldc_pad (extra
leading-dimension elements of every output), off (C / Z / R start one element past a 16-B boundary), c8 ("e4m3" / "e5m2": the
epilogue emits C as fp8 bytes under a delayed scale whose previous amax is c8_amax)."""
from __future__ import annotations

import ctypes as C

V_PAD = 250112  # the LM head's padded vocabulary (250 054 valid columns)


def case(name, M, N, K, *, akm=False, bkm=False, dtype="bf16", cus=0, plan=None, kernel="", tags=(), group=None, **feats):
    return dict(name=name, M=M, N=N, K=K, akm=akm, bkm=bkm, dtype=dtype, cus=cus, plan=plan, kernel=kernel, tags=tuple(tags),
                group=group, feats=feats)


def P(tile, tile_m, kgroups, phased, grid, blocks_per_cu):
    return dict(tile=tile, tile_m=tile_m, kgroups=kgroups, phased=phased, grid=grid, blocks_per_cu=blocks_per_cu)


CASES = [
    # ---- ViT (3200 rows, width 768, ffn 3072)
    case("vit_fc1_fwd_quickgelu", 3200, 3072, 768, bias=1, act=3, zout=1, plan=P(128, 192, 1, 0, 408, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,false,1,false,0>", tags=("t192",)),
    case("vit_fc1_dx_dquickgelu", 3200, 3072, 768, bkm=True, dact=3, plan=P(128, 192, 1, 0, 408, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,true,1,false,0>", tags=("t192",)),
    case("vit_fc2_fwd_residual", 3200, 768, 3072, bias=1, res=1, plan=P(128, 128, 2, 0, 150, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,true,0>", tags=("kg128",)),
    case("vit_dw_qkv_rowsum", 768, 768, 3200, akm=True, bkm=True, c32=1, rowsum=1, plan=P(64, 64, 4, 0, 144, 1),
         kernel="gemm_bf16_kernel<32,32,2,64,true,true,4,true,0>", tags=("kg", "tile")),
    case("vit_dw_fc1_rowsum", 3072, 768, 3200, akm=True, bkm=True, c32=1, rowsum=1, plan=P(128, 128, 2, 0, 144, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,true,true,2,true,0>", tags=("kg128", "tile")),
    # ---- packed decoder (2404 valid rows of 2432, d 1024, ffn 4096)
    case("dec_qkv_fwd", 2404, 3072, 1024, bias=1, plan=P(128, 128, 1, 0, 456, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,true,0>", tags=("kg128", "tile")),
    case("dec_out_fwd_dropout_residual", 2404, 1024, 1024, bias=1, drop=0.1, res=1, plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,true,0>", tags=("kg128",)),
    case("dec_fc1_fwd_gelu_dropout", 2404, 4096, 1024, bias=1, act=1, zout=1, drop=0.5, plan=P(128, 192, 1, 0, 416, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,false,1,false,0>", tags=("t192",)),
    case("dec_fc1_fwd_bias", 2404, 4096, 1024, bias=1, plan=P(128, 192, 1, 0, 416, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,false,1,true,0>", tags=("t192",)),
    case("dec_fc2_dx", 2404, 1024, 4096, bkm=True, plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,true,2,true,0>", tags=("kg128",)),
    case("dec_dw_fc_kvalid_stale", 4096, 1024, 2432, akm=True, bkm=True, c32=1, rowsum=1, rowsum_k=2404, k_valid=2404,
         plan=P(128, 128, 2, 0, 256, 1), kernel="gemm_bf16_kernel<64,32,4,64,true,true,2,true,0>", tags=("kg128",)),
    case("dec_dw_grouped_kvalid", 0, 0, 0, akm=True, bkm=True, plan=P(128, 128, 1, 0, 512, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,true,true,1,true,0>", tags=("kg128",),
         group=[dict(M=4096, N=1024, K=2432, c32=1, rowsum=1, rowsum_k=2404, k_valid=2404),
                dict(M=1024, N=4096, K=2432, c32=1, k_valid=2404)]),
    case("dec_dx_accumulate_256", 3200, 4096, 1024, bkm=True, acc=1, plan=P(256, 256, 1, 0, 208, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,true,1,false,0>", tags=("tile", "persist")),
    # ---- 256 x 256 NT: phased / four-wave / two-blocks-per-CU kernels
    case("dec_fc1_fwd_256_gelu", 3200, 4096, 1024, bias=1, act=2, zout=1, plan=P(256, 256, 1, 2, 208, 1),
         kernel="gemm_phased_kernel<false,false,false>", tags=("w4", "tile")),
    case("cross_kv_all_layers", 3200, 24576, 1024, bias=1, plan=P(256, 256, 1, 2, 1248, 1),
         kernel="gemm_w4_kernel<2>", tags=("w4", "d2", "tile", "persist")),
    case("head_dE_nt_f32", 16384, 1024, 2432, c32=1, plan=P(256, 256, 1, 2, 256, 1),
         kernel="gemm_w4_kernel<8>", tags=("w4", "d2", "tile")),
    case("head_dX_split_slabs_6", 2404, 1024, 16384, c32=1, split=6, slabs=1, plan=P(256, 256, 1, 2, 240, 1),
         kernel="gemm_w4_kernel<8>", tags=("w4", "d2", "tile")),
    case("head_fwd_rowstat", 2404, V_PAD, 1024, bias=1, rowstat=1, nvalid=250054, plan=P(128, 256, 1, 2, 19540, 2),
         kernel="gemm_d2_kernel<1>", tags=("w4", "d2")),
    case("head_dE_tn_rowsum_persistent", V_PAD, 1024, 2432, akm=True, bkm=True, c32=1, rowsum=1, rowsum_k=2404, k_valid=2404,
         plan=P(256, 256, 1, 0, 256, 1), kernel="gemm_bf16_kernel<128,64,4,64,true,true,1,true,0>", tags=("persist", "tile")),
    # ---- decode (1024 rows = 256 images x 4 beams)
    case("decode_self_qkv", 1024, 1024, 1024, bias=1, plan=P(64, 64, 4, 0, 256, 1),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,4,true,0>", tags=("kg", "tile")),
    case("decode_fc1_gelu", 1024, 4096, 1024, bias=1, act=1, plan=P(128, 128, 2, 0, 256, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128", "tile")),
    case("decode_ln_fold", 1024, 1024, 1024, ln=1, plan=P(64, 64, 4, 0, 256, 1),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,4,true,0>", tags=("kg", "tile")),
    case("decode_out_rowsum2_residual", 1024, 1024, 1024, bias=1, res=1, rowsum2=1, plan=P(64, 64, 4, 0, 256, 1),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,4,true,0>", tags=("kg", "tile")),
    case("decode_cross_ln_fold_256", 1024, 32768, 1024, ln=1, plan=P(256, 256, 1, 2, 512, 1),
         kernel="gemm_w4_kernel<6>", tags=("w4", "d2", "tile")),
    # ---- fp8 (e4m3 activations / weights, e5m2 gradients)
    case("fp8_fc1_fwd_256", 3200, 4096, 1024, dtype="e4m3", bias=1, plan=P(256, 256, 1, 0, 208, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,false,1,true,1>", tags=("tile",)),
    case("fp8_dx_256_dgelu", 3200, 4096, 1024, dtype="e5m2", dact=1, plan=P(256, 256, 1, 0, 208, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,false,1,false,2>", tags=("tile",)),
    case("fp8_dw_tn_256", 4096, 4096, 3200, akm=True, bkm=True, dtype="e5m2", c32=1, k_valid=3104, plan=P(256, 256, 1, 0, 256, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,true,true,1,true,2>", tags=("tile", "persist")),
    case("fp8_fc1_fwd_gelu_128", 2404, 4096, 1024, dtype="e4m3", bias=1, act=1, zout=1, plan=P(128, 128, 1, 0, 608, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,false,1>", tags=("kg128", "tile")),
    case("fp8_dx_dgelu_128", 2404, 4096, 1024, dtype="e5m2", dact=2, plan=P(128, 128, 1, 0, 608, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,false,2>", tags=("kg128", "tile")),
    case("fp8_fc1_fwd_bias_128", 2404, 4096, 1024, dtype="e4m3", bias=1, plan=P(128, 128, 1, 0, 608, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,true,1>", tags=("kg128", "tile")),
    case("fp8_out_kg2_e4m3", 2404, 1024, 1024, dtype="e4m3", bias=1, res=1, plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,true,1>", tags=("kg128",)),
    case("fp8_dx_kg2_e5m2", 2404, 1024, 1024, dtype="e5m2", plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,true,2>", tags=("kg128",)),
    case("fp8_dw_grouped_tn", 0, 0, 0, akm=True, bkm=True, dtype="e5m2", plan=P(128, 128, 1, 0, 512, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,true,true,1,true,2>", tags=("kg128",),
         group=[dict(M=4096, N=1024, K=2432, c32=1, k_valid=2404), dict(M=1024, N=4096, K=2432, c32=1, k_valid=2404)]),
    case("fp8_dx_split_slabs_8", 2404, 1024, 4096, dtype="e5m2", c32=1, split=8, slabs=1, plan=P(256, 256, 1, 0, 320, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,false,1,false,2>", tags=("tile",)),
    # fp8 C emission (the product's GELU(FFN-in) -> e4m3 operand of FFN-out and dGELU-scaled dX of FFN-out -> e5m2 dy of FFN-in)
    case("fp8c_fc1_gelu_e4m3", 2404, 4096, 1024, dtype="e4m3", bias=1, act=1, zout=1, c8="e4m3", c8_amax=96.0,
         plan=P(128, 128, 1, 0, 608, 2), kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,false,1>", tags=("kg128", "tile")),
    case("fp8c_fc2_dx_dgelu_e5m2", 2404, 1024, 4096, dtype="e5m2", dact=1, c8="e5m2", c8_amax=160.0,
         plan=P(128, 128, 2, 0, 152, 1), kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,2>", tags=("kg128",)),
    case("fp8c_decode_gelu_64", 1024, 1024, 1024, dtype="e4m3", bias=1, act=2, zout=1, c8="e4m3", c8_amax=80.0,
         plan=P(64, 64, 2, 0, 256, 2), kernel="gemm_bf16_kernel<32,32,2,64,false,false,2,false,1>", tags=("kg", "tile")),
    # ---- features the product does not launch today (header-admitted)
    case("alpha_bias_act_dropout_res", 2404, 1024, 1024, alpha=0.375, bias=1, act=2, zout=1, drop=0.5, res=1,
         plan=P(128, 128, 2, 0, 152, 1), kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128",)),
    case("alpha_dact_accumulate_f32", 1024, 1024, 1024, alpha=-1.5, dact=1, acc=1, c32=1, plan=P(64, 64, 4, 0, 256, 1),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,4,false,0>", tags=("kg",)),
    case("alpha_256_persistent", 3200, 24576, 1024, alpha=0.625, bias=1, res=1, plan=P(256, 256, 1, 0, 256, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,true,1,true,0>", bkm=True, tags=("tile", "persist")),
    case("alpha_w4_bare", 3200, 24576, 1024, alpha=0.625, bias=1, plan=P(256, 256, 1, 2, 1248, 1), kernel="gemm_w4_kernel<2>",
         tags=("w4", "d2")),
    case("alpha_w4_f32_slabs", 2404, 1024, 16384, alpha=-0.75, c32=1, split=6, slabs=1, plan=P(256, 256, 1, 2, 240, 1),
         kernel="gemm_w4_kernel<8>", tags=("w4", "d2")),
    case("alpha_d2_rowstat", 2404, 65536, 1024, alpha=0.875, bias=1, rowstat=1, nvalid=65500, plan=P(128, 256, 1, 2, 5120, 2),
         kernel="gemm_d2_kernel<1>", tags=("w4", "d2")),
    case("alpha_phased_gelu", 3200, 4096, 1024, alpha=1.5, bias=1, act=1, zout=1, plan=P(256, 256, 1, 2, 208, 1),
         kernel="gemm_phased_kernel<false,false,false>", tags=("w4",)),
    case("alpha_t192_residual", 2404, 4096, 1024, alpha=0.5, bias=1, res=1, plan=P(128, 192, 1, 0, 416, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,false,1,true,0>", tags=("t192",)),
    case("alpha_fp8_256", 3200, 4096, 1024, dtype="e4m3", alpha=-0.625, bias=1, plan=P(256, 256, 1, 0, 208, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,false,1,true,1>", tags=("tile",)),
    case("alpha_fp8_c8_128", 2404, 4096, 1024, dtype="e4m3", alpha=0.75, act=3, c8="e4m3", c8_amax=48.0, plan=P(128, 128, 1, 0, 608, 2),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,1,false,1>", tags=("kg128",)),
    case("split_atomic_4", 1024, 1024, 2048, c32=1, split=4, plan=P(128, 128, 2, 0, 256, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128",)),
    case("split_slabs_3_kmajor", 1024, 1024, 2048, akm=True, bkm=True, c32=1, split=3, slabs=1, k_valid=1900, plan=P(128, 128, 2, 0, 192, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,true,true,2,false,0>", tags=("kg128",)),
    case("scalar_path_n_odd_ldc", 3200, 3069, 768, bias=1, act=3, zout=1, ldc_pad=3, plan=P(128, 192, 1, 0, 408, 2),
         kernel="gemm_bf16_kernel<96,32,4,64,false,false,1,false,0>", tags=("t192",)),
    case("scalar_path_f32_residual_256", 3200, 4096, 1024, bkm=True, bias=1, res=1, c32=1, plan=P(256, 256, 1, 0, 208, 1),
         kernel="gemm_bf16_kernel<128,64,4,64,false,true,1,false,0>", tags=("tile",)),
    case("scalar_path_dact_accumulate_bf16", 2404, 1024, 1024, dact=2, acc=1, plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128",)),
    case("misaligned_c_z_r", 2404, 1024, 1024, bias=1, act=1, zout=1, res=1, off=1, plan=P(128, 128, 2, 0, 152, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128",)),
    case("misaligned_dact_128", 1024, 4096, 1024, dact=1, res=1, off=1, plan=P(128, 128, 2, 0, 256, 1),
         kernel="gemm_bf16_kernel<64,32,4,64,false,false,2,false,0>", tags=("kg128",)),
    case("grouped_mixed_plain_tiles", 0, 0, 0, plan=P(64, 64, 1, 0, 117, 4), tags=("kg",),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,1,false,0>",
         group=[dict(M=512, N=256, K=256, bias=1), dict(M=200, N=136, K=256, act=2, zout=1), dict(M=64, N=64, K=256, res=1),
                dict(M=320, N=512, K=256, acc=1, c32=1), dict(M=96, N=1000, K=256, bias=1, drop=0.1)]),
    case("grouped_eleven", 0, 0, 0, akm=True, bkm=True, plan=P(64, 64, 1, 0, 30, 4), tags=("kg",),
         kernel="gemm_bf16_kernel<32,32,2,64,true,true,1,true,0>",
         group=[dict(M=64 * (1 + i % 3), N=128, K=320, c32=1, rowsum=1, k_valid=300 - 5 * i) for i in range(11)]),
    # ---- ragged edges, one K-tile
    case("edge_m1_n1", 1, 1, 64, bias=1, plan=P(64, 64, 1, 0, 1, 4), kernel="gemm_bf16_kernel<32,32,2,64,false,false,1,false,0>",
         tags=("kg",)),
    case("edge_m63_n65", 63, 65, 64, bias=1, act=1, zout=1, plan=P(64, 64, 1, 0, 2, 4),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,1,false,0>", tags=("kg",)),
    case("edge_m129_n127", 129, 127, 128, bias=1, res=1, plan=P(64, 64, 1, 0, 6, 4),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,1,false,0>", tags=("kg",)),
    case("edge_m120_n248_kmajor", 120, 248, 64, akm=True, bkm=True, c32=1, rowsum=1, k_valid=40, plan=P(64, 64, 1, 0, 8, 4),
         kernel="gemm_bf16_kernel<32,32,2,64,true,true,1,true,0>", tags=("kg",)),
    case("edge_m257_n255_256tile", 257, 255, 64, bias=1, cus=0, plan=P(64, 64, 1, 0, 20, 4),
         kernel="gemm_bf16_kernel<32,32,2,64,false,false,1,false,0>", tags=("tile",)),
]

# budgets under which the persistent 256^2 grid and the K-group variants run with their results checked
CU_BUDGETS = (256, 248, 192, 128, 64)
BUDGET_CASES = ("head_dE_tn_rowsum_persistent", "alpha_256_persistent", "vit_dw_qkv_rowsum", "dec_out_fwd_dropout_residual",
                "decode_self_qkv", "dec_dw_fc_kvalid_stale")

# the library latches these switches at its first GEMM: the GPU module reruns the cases they can change in a child process each
SWITCHES = [("MIC_GEMM_W4", "0", "w4"), ("MIC_GEMM_D2", "0", "d2"), ("MIC_GEMM_D2", "2", "d2"), ("MIC_GEMM_T192", "0", "t192"),
            ("MIC_GEMM_PERSIST", "0", "persist"), ("MIC_GEMM_TILE", "64", "tile"), ("MIC_GEMM_TILE", "128", "tile"),
            ("MIC_GEMM_TILE", "256", "tile"), ("MIC_GEMM_KG", "1", "kg"), ("MIC_GEMM_KG", "2", "kg"), ("MIC_GEMM_KG", "4", "kg"),
            ("MIC_GEMM_KG128", "1", "kg128"), ("MIC_GEMM_KG128", "2", "kg128")]

BY_NAME = {c["name"]: c for c in CASES}


def ld_of(N, f) -> int:
    """leading dimension of every output of a problem: past N by 8 elements, or by `ldc_pad`"""
    return N + f.get("ldc_pad", 8)


def problems(c):
    """[(M, N, K, feats)] of a case (one entry unless grouped)"""
    if c["group"]:
        return [(g["M"], g["N"], g["K"], {k: v for k, v in g.items() if k not in ("M", "N", "K")}) for g in c["group"]]
    return [(c["M"], c["N"], c["K"], c["feats"])]


def plan_args(c):
    """mic_gemm_args of a case for mic_gemm_plan: the fields the planner reads, with stand-in (never dereferenced) pointers"""
    from mic_amd import _lib as L

    fake = 1 << 24
    f8 = c["dtype"] != "bf16"
    arr = (L.GemmArgs * len(problems(c)))()
    for g, (M, N, K, f) in zip(arr, problems(c)):
        g.dtype = L.MIC_FP8 if f8 else L.MIC_BF16
        g.c_dtype = L.MIC_FP8 if f.get("c8") else (L.MIC_F32 if f.get("c32") else L.MIC_BF16)
        g.a_fmt = L.MIC_E5M2 if c["dtype"] == "e5m2" else L.MIC_E4M3
        g.M, g.N, g.K, g.a_kmajor, g.b_kmajor = M, N, K, int(c["akm"]), int(c["bkm"])
        off = 2 if f.get("off") else 0
        g.A = g.B = fake
        g.lda, g.ldb = (M if c["akm"] else K), (N if c["bkm"] else K)
        g.C, g.ldc = fake + off, ld_of(N, f)
        g.bias = fake if f.get("bias") or f.get("ln") else None
        g.act, g.dact = f.get("act", 0), f.get("dact", 0)
        if f.get("zout") or f.get("dact"):
            g.Zout = fake + off if f.get("zout") else None
            g.Zin = fake + off if f.get("dact") else None
            g.ldz = g.ldc
        if f.get("res"):
            g.R, g.ldr = fake + off, g.ldc
        g.accumulate = int(bool(f.get("acc")))
        g.dropout_p, g.alpha = float(f.get("drop", 0.0)), float(f.get("alpha", 0.0))
        g.split_k = f.get("split", 0)
        g.split_stride = (M * g.ldc + 63) // 64 * 64 if f.get("slabs") else 0
        g.a_rowsum = fake if f.get("rowsum") else None
        g.rowstat = fake if f.get("rowstat") else None
        g.k_valid = f.get("k_valid", 0)
        if f.get("ln"):
            g.a_ln_stats, g.a_ln_colsum, g.a_ln_width = fake, fake, K
        g.rowsum2 = fake if f.get("rowsum2") else None
    return arr


def kernel_name(rep: dict, dtype: str, akm, bkm) -> str:
    """the kernel instantiation a plan report (mic_gemm_plan: family, tiling, K-groups, PLAIN, epilogue variant) names, as the
    kernel traces print it (without blanks)"""
    from mic_amd import _lib as L

    b = lambda x: "true" if x else "false"  # noqa: E731
    fam = L.GEMM_FAMILIES[rep["family"]]
    if fam in ("w4", "d2"):
        return f"gemm_{fam}_kernel<{rep['epi']}>"
    if fam == "phased":
        return f"gemm_phased_kernel<{b(akm)},{b(bkm)},{b(rep['plain'])}>"
    wn, wnw = {256: (64, 4), 128: (32, 4), 64: (32, 2)}[rep["tile"]]
    f8 = {"bf16": 0, "e4m3": 1, "e5m2": 2}[dtype]
    return f"gemm_bf16_kernel<{rep['tile_m'] // 2},{wn},{wnw},64,{b(akm)},{b(bkm)},{rep['kgroups']},{b(rep['plain'])},{f8}>"


def switch_honoured(switch: str, c, got: dict) -> bool:
    """does the report `got` (every field of mic_gemm_plan under the latched switch) follow MIC_GEMM_*=value for case c?"""
    from mic_amd import _lib as L

    env, val = switch.split("=")
    v = int(val)
    fp8 = c["dtype"] != "bf16"
    f = c["feats"]
    fam = L.GEMM_FAMILIES[got["family"]]
    if env == "MIC_GEMM_TILE":
        if f.get("rowstat"):
            return True  # softmax partials force the 256-wide configuration
        want = 128 if (fp8 and v == 64 and c["akm"]) or (f.get("c8") and v == 256) else v
        return got["tile"] == want and got["tile_m"] == want
    if env == "MIC_GEMM_KG":
        return got["tile"] != 64 or got["kgroups"] == v
    if env == "MIC_GEMM_KG128":
        return not (got["tile"] == 128 and got["tile_m"] == 128) or got["kgroups"] == v
    if env == "MIC_GEMM_T192":
        return got["tile_m"] != 192 and fam != "t192"
    if env == "MIC_GEMM_PERSIST":
        return got["grid"] == got["blocks"]
    if env == "MIC_GEMM_W4":
        return got["phased"] != 2 and fam not in ("w4", "d2")  # (the default MIC_GEMM_D2=3 only takes what the four-wave kernel would)
    if env == "MIC_GEMM_D2":
        d2_tiling = got["tile"] == 128 and got["tile_m"] == 256
        if v == 0:
            return fam != "d2" and not d2_tiling
        # 2: every single-problem bf16 NT launch with 256-row tiles whose epilogue gemm_d2.hip covers (no folded LayerNorm, no rowsum2,
        # whole 8-column units with 16-B aligned rows everywhere)
        nt1 = not fp8 and not c["akm"] and not c["bkm"] and not c["group"] and got["tile_m"] == 256
        want = nt1 and not (f.get("ln") or f.get("rowsum2") or f.get("off")) and ld_of(c["N"], f) % 8 == 0 and c["N"] % 8 == 0
        return (fam == "d2") == bool(want) and d2_tiling == (fam == "d2")
    raise AssertionError(switch)


def plan_report(c) -> dict:
    """every field of mic_gemm_plan's report for a case"""
    from mic_amd import _lib as L

    arr = plan_args(c)
    out = L.GemmPlanInfo()  # (a group of more than 8 problems: the plan of its first launch)
    L.check(L.lib().mic_gemm_plan(arr, min(len(arr), 8), C.byref(out)), "mic_gemm_plan")
    return {k: getattr(out, k) for k, _ in L.GemmPlanInfo._fields_}


def plan_of(c) -> dict:
    rep = plan_report(c)
    return {k: rep[k] for k in ("tile", "tile_m", "kgroups", "phased", "grid", "blocks_per_cu")}


# ---- the recorded planner sweep (tests/golden/gemm_plan_parent.npz, written by tests/golden/make_golden_gemm_plan.py on the commit
# before the dispatch decision moved into one function): drawn argument sets and that commit's mic_gemm_plan answers.
#   draws  [n][7]: first problem row, problem count, dtype (0 bf16, 1 e4m3, 2 e5m2), a_kmajor, b_kmajor, CU budget (0 = default),
#                  switch block (0 = default switches, i + 1 = SWITCHES[i])
#   probs  [m][8]: M, N, K, ldc, feature bits (F_*), activation id (act, or dact with F_DACT), split_k, fp8-C format + 1 (0 = none)
#   answers [n][9]: return code and the eight fields of ANSWER_FIELDS
PLAN_FIXTURE = "golden/gemm_plan_parent.npz"
F_C32, F_BIAS, F_ZOUT, F_DACT, F_RES, F_ACC, F_ROWSTAT, F_ROWSUM, F_OFF, F_SLABS = (1 << i for i in range(10))
ANSWER_FIELDS = ("tile", "kgroups", "blocks", "grid", "blocks_per_cu", "phased", "cu_budget", "tile_m")


def draw_args(d, probs):
    """mic_gemm_args of one recorded draw (stand-in pointers, never dereferenced; every argument set passes mic_gemm's host checks)"""
    from mic_amd import _lib as L

    fake = 1 << 24
    first, count, dt, akm, bkm = (int(x) for x in d[:5])
    arr = (L.GemmArgs * count)()
    for g, row in zip(arr, probs[first:first + count]):
        M, N, K, ldc, fl, actid, split, c8 = (int(x) for x in row)
        g.dtype = L.MIC_FP8 if dt else L.MIC_BF16
        g.c_dtype = L.MIC_FP8 if c8 else (L.MIC_F32 if fl & F_C32 else L.MIC_BF16)
        g.a_fmt, g.b_fmt = (L.MIC_E5M2 if dt == 2 else L.MIC_E4M3), L.MIC_E4M3
        g.M, g.N, g.K, g.a_kmajor, g.b_kmajor = M, N, K, akm, bkm
        g.A, g.lda, g.B, g.ldb = fake, (M if akm else K), fake, (N if bkm else K)
        off = 2 if fl & F_OFF else 0
        g.C, g.ldc = fake + off, ldc
        g.bias = fake if fl & F_BIAS else None
        g.act, g.dact = (0, actid) if fl & F_DACT else (actid, 0)
        g.Zout = fake + off if fl & F_ZOUT else None
        g.Zin = fake + off if fl & F_DACT else None
        g.ldz = ldc
        if fl & F_RES:
            g.R, g.ldr = fake + off, ldc
        g.accumulate = int(bool(fl & F_ACC))
        g.split_k = split
        g.split_stride = (M * ldc + 63) // 64 * 64 if fl & F_SLABS else 0
        g.a_rowsum = fake if fl & F_ROWSUM else None
        if fl & F_ROWSTAT:
            g.rowstat, g.rowstat_ld = fake, N // 64
        if c8:
            g.c_q8_state, g.c_q8_fmt = fake, c8 - 1
    return arr


def plan_answers(draws, probs, rows):
    """[rc, *ANSWER_FIELDS] of mic_gemm_plan for the draws `rows`, each under its recorded CU budget (this process's latched switches)"""
    from mic_amd import _lib as L

    lib = L.lib()
    out = []
    try:
        for r in rows:
            d = draws[r]
            L.check(lib.mic_set_cu_budget(int(d[5])), "mic_set_cu_budget")
            info = L.GemmPlanInfo()
            rc = lib.mic_gemm_plan(draw_args(d, probs), int(d[1]), C.byref(info))
            out.append([rc] + [getattr(info, k) for k in ANSWER_FIELDS])
    finally:
        lib.mic_set_cu_budget(0)
    return out


if __name__ == "__main__":  # child process of the equivalence test: replay one switch block, print the rows that differ
    import json
    import os
    import sys

    import numpy as np

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    fx = np.load(os.path.join(here, PLAN_FIXTURE))
    block = int(sys.argv[1])
    rows = np.nonzero(fx["draws"][:, 6] == block)[0]
    got = plan_answers(fx["draws"], fx["probs"], rows)
    bad = [(int(r), g, fx["answers"][r].tolist()) for r, g in zip(rows, got) if g != fx["answers"][r].tolist()]
    ignored = []  # ... and the conformance cases this block's switch can change: does the report follow the switch?
    if block:
        env, val, tag = SWITCHES[block - 1]
        ignored = [c["name"] for c in CASES if tag in c["tags"] and not switch_honoured(f"{env}={val}", c, plan_report(c))]
    print(json.dumps({"replayed": len(rows), "differ": len(bad), "first": bad[:5], "switch_ignored": ignored}))
