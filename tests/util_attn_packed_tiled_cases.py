"""The case table of tests/test_attn_packed_tiled_gpu.py: packed (variable-length) rows through the TILED attention kernels
(mic_attn_fwd_packed_tiled / mic_attn_bwd_packed_tiled: attn_fwd_tiled_kernel, attn_bwd_tiled_kernel<T, 0 / 1> with a PackedRows
argument).  The smallest shapes at which the block logic can go wrong: lengths on either side of the 64-row block edges, a last
block of one or two rows, sequences that leave whole blocks of the grid without work, and the tiled kernels on a one-tile shape.
Operands come from tests/util_attn_cases.py::packed_inputs (same generator, same layouts as the one-tile packed cases)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import util_attn_cases as AC  # noqa: E402

DTYPES = AC.DTYPES
packed_inputs = AC.packed_inputs


def _p(name, H, Tq_max, Tk, q_len, kv_packed, dense_twin=False):
    """self-attention: kv_packed, causal, the fused [rows][3d] layout; cross-attention: dense keys, not causal, k | v in [rows][2d]"""
    return dict(name=name, B=len(q_len), H=H, Tq_max=Tq_max, Tk=Tk, q_len=list(q_len), kv_packed=kv_packed, causal=bool(kv_packed),
                layout="fused3" if kv_packed else "kv2", dense_twin=dense_twin, claim="tiled")


SELF = [
    _p("pt_self_65", 2, 65, 65, (1, 64, 65, 33), 1),
    _p("pt_self_128", 3, 128, 128, (128, 1, 64, 65, 127, 128, 9), 1),
    _p("pt_self_130", 2, 130, 130, (130, 129, 3, 64), 1),               # three query blocks, the last two rows long
    _p("pt_self_200", 2, 200, 200, (200, 1, 137, 64, 192), 1),
    _p("pt_self_48", 3, 48, 48, (48, 1, 33), 1),                         # the tiled kernels on a one-tile shape
]
CROSS = [
    _p("pt_cross_128x50", 3, 128, 50, (128, 1, 65, 64, 40), 0),          # the product's shape at seq 128
    _p("pt_cross_65x64", 2, 65, 64, (65, 1, 64), 0),
    _p("pt_cross_64x197", 2, 64, 197, (64, 1, 33), 0),                   # ViT-B/16: one query block, four key blocks
    _p("pt_cross_130x197", 2, 130, 197, (130, 65, 7), 0),
]
# every sequence full: bit for bit what mic_attn_fwd / mic_attn_bwd give on the same rows
TWINS = [
    _p("pt_twin_self_128", 2, 128, 128, (128, 128, 128), 1, dense_twin=True),
    _p("pt_twin_self_130", 2, 130, 130, (130, 130), 1, dense_twin=True),
    _p("pt_twin_cross_128x50", 3, 128, 50, (128, 128, 128), 0, dense_twin=True),
]
CASES = SELF + CROSS + TWINS
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def product_lengths(B=64, T=128):
    """caption lengths of one benchmark batch at seq_len T (bench.synth_batch: n ~ U{8..T-2} tokens + language code + eos)"""
    import bench

    mask = bench.synth_batch(B, T, 1000, 1, seed=128)["attention_mask"]
    ql = mask.sum(1).astype(np.int64)
    assert (mask[np.arange(B), ql - 1] == 1).all() and ql.min() >= 10 and ql.max() <= T
    return [int(n) for n in ql]


def product_case(kind):
    """B 64, H 16, Tq_max 128 on the lengths of a benchmark batch: self-attention, or cross-attention over 50 keys"""
    ql = product_lengths()
    return _p(f"pt_product_{kind}", 16, 128, 128 if kind == "self" else 50, ql, 1 if kind == "self" else 0)
