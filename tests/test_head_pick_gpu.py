"""The head GEMM without C (gemm_d2_kernel<2>: softmax partials and each row's picked value, no logits stored) and the two row
kernels behind `score`, at the smallest shapes where the epilogue can go wrong: one row, rows that end inside a 32-row pass, one
whole 256-row tile, a second tile; one and several 128-column tiles with a ragged last granule; two K depths.

Run A = the existing launch (C and rowstat) + mic_ce_rows_tiles; run B = the pick launch with C = None on fresh, poisoned buffers +
mic_ce_rows_picked.  Everything B leaves must have A's bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # rows behind row M that no launch may touch


def _labels(M, V, g):
    fixed = [c for c in (0, V - 1, 63, 64, 127, 128, 255, 256, 7, 8, 56) if c < V]
    lab = torch.randint(0, V, (M,), generator=g, dtype=torch.int64)
    n = min(M, len(fixed))
    lab[:n] = torch.tensor(fixed[:n])
    return lab.to(torch.int32)


def test_label_list_covers_the_unit_and_tile_edges():
    """the label list of the largest case has a label in the first and in the last 8-column unit of a granule, and on both sides of a
    128-column tile edge"""
    lab = _labels(300, 1003, torch.Generator().manual_seed(0)).tolist()
    assert any(c % 64 < 8 for c in lab) and any(c % 64 >= 56 for c in lab)
    assert 127 in lab and 128 in lab and 255 in lab and 256 in lab and 0 in lab and 1002 in lab and 63 in lab and 64 in lab


@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("V,Vpad", [(250, 256), (1003, 1024)])
@pytest.mark.parametrize("M", [1, 37, 256, 300])
def test_pick_launch_has_the_bits_of_the_materialised_head(dev, M, V, Vpad, K):
    from mic_amd import ops

    g = torch.Generator().manual_seed(1000 * M + V + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    b = (torch.randn(Vpad, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    bias = torch.randn(Vpad, generator=g).to(dev)
    lab = _labels(M, V, g).to(dev)
    assert ops.gemm_plan([(M, Vpad, K)], kernel=True, pick=True)["epi"] == 2
    nan = float("nan")
    # run A
    c_a = torch.zeros(M + GUARD, Vpad, dtype=torch.bfloat16, device=dev)
    stat_a = torch.full((M + GUARD, 2 * (Vpad // 64)), nan, dtype=torch.float32, device=dev)
    ops.gemm(a, b, c_a, M, Vpad, K, bias=bias, rowstat=stat_a, rowstat_nvalid=V)
    lse_a, rl_a = torch.full((M,), nan, device=dev), torch.full((M,), nan, device=dev)
    ops.ce_rows_tiles(c_a, Vpad, V, stat_a, lab, lse_a, rl_a, M)
    # run B: fresh buffers, NaN everywhere; a poisoned C-sized bystander that is never passed to the launch
    stat_b = torch.full((M + GUARD, 2 * (Vpad // 64)), nan, dtype=torch.float32, device=dev)
    pick = torch.full((M + GUARD,), nan, dtype=torch.float32, device=dev)
    bystander = torch.full((M + GUARD, Vpad), nan, dtype=torch.bfloat16, device=dev)
    ops.gemm(a, b, None, M, Vpad, K, bias=bias, rowstat=stat_b, rowstat_nvalid=V, pick_col=lab, pick_out=pick)
    lse_b, rl_b = torch.full((M,), nan, device=dev), torch.full((M,), nan, device=dev)
    ops.ce_rows_picked(V, stat_b, pick, lse_b, rl_b, M)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.isfinite(stat_b[:M]).all() and torch.isfinite(pick[:M]).all()
    assert torch.equal(bits(stat_b[:M]), bits(stat_a[:M]))
    want = c_a[:M].gather(1, lab.long()[:, None])[:, 0].float()
    assert torch.equal(bits(pick[:M]), bits(want)), (pick[:M] - want).abs().max().item()
    assert torch.equal(bits(lse_b), bits(lse_a)) and torch.equal(bits(rl_b), bits(rl_a)) and torch.isfinite(rl_b).all()
    # the guard behind row M is untouched, and nothing stored a C
    assert torch.isnan(stat_b[M:]).all() and torch.isnan(pick[M:]).all() and torch.isnan(stat_a[M:]).all()
    assert torch.isnan(bystander).all()
    # the picked launch WITH a C stores the same C as run A
    c_b = torch.zeros(M + GUARD, Vpad, dtype=torch.bfloat16, device=dev)
    pick2 = torch.full((M + GUARD,), nan, dtype=torch.float32, device=dev)
    ops.gemm(a, b, c_b, M, Vpad, K, bias=bias, rowstat=stat_b, rowstat_nvalid=V, pick_col=lab, pick_out=pick2)
    torch.cuda.synchronize()
    assert torch.equal(c_b.view(torch.int16), c_a.view(torch.int16)) and torch.equal(bits(pick2[:M]), bits(want)) and torch.isnan(pick2[M:]).all()
    # fp64 anchor: the row losses are cross-entropies of the stored logits
    ref = torch.logsumexp(c_a[:M, :V].double(), 1) - want.double()
    assert torch.allclose(rl_b.double(), ref, rtol=1e-5, atol=1e-5)


def test_segment_sums(dev):
    from mic_amd import ops

    lens = [0, 1, 63, 64, 65, 1000, 0, 5]
    gap = 3  # poisoned elements between the segments
    g = torch.Generator().manual_seed(5)
    off, pos, x = [], gap, []
    x.append(torch.full((gap,), float("nan")))
    for n in lens:
        off.append(pos)
        x.append(torch.randn(n, generator=g) * 3.0)
        x.append(torch.full((gap,), float("nan")))
        pos += n + gap
    x = torch.cat(x)
    xd = x.to(dev)
    d_off, d_len = torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((len(lens) + 4,), float("nan"), device=dev)
        ops.segment_sums(d_off, d_len, xd, out, len(lens), scale=-1.0)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][: len(lens)].view(torch.int32), outs[1][: len(lens)].view(torch.int32)) and torch.isnan(outs[0][len(lens):]).all()
    got = outs[0].cpu()
    for s, (o, n) in enumerate(zip(off, lens)):
        seg = x[o: o + n].double()
        bound = n * 2.0 ** -24 * seg.abs().sum().item()
        assert abs(got[s].item() + seg.sum().item()) <= bound, (s, n, got[s].item(), -seg.sum().item(), bound)
        if n == 0:
            assert got[s].view(torch.int32).item() == 0  # +0, not -0
    # the same segments, one launch per segment (another grid): the same bits
    for s in range(len(lens)):
        one = torch.full((1,), float("nan"), device=dev)
        ops.segment_sums(d_off[s: s + 1], d_len[s: s + 1], xd, one, 1, scale=-1.0)
        assert one.view(torch.int32).item() == outs[0][s].view(torch.int32).item()
