"""mic_sample_rows_keyed (csrc/sample_keyed.hip): several categorical draws per image in one launch, each with its own key read from device
memory, and the log-probability of every draw.

  * draws = 1 is mic_sample_rows bit for bit (same device functions, noise skipped only where the sum is -inf anyway);
  * draws > 1: rows n::draws are a mic_sample_rows call over the images with keys[n] — and, where the fp64 order is decisive
    (util_decode_ref.sample_ref), the fp64 reference's draw;
  * score += log p(drawn) against fp64 within the bound util_decode_ref derives for an fp32 log-sum-exp of the row: lse_ref's e_ls
    with n_r = the rescales one addend can pass through in THIS kernel — every later entry of its thread may raise the thread's
    maximum (ceil(V / 1024) entries of the 16-byte body + one head + one tail entry), then 6 shuffle levels and 15 wave merges —
    plus one rounding each of v - max and of the final difference: b = e_ls + u32 (|v - M| + |log p|), proc_ref's form.
"""
import math

import numpy as np
import pytest
import torch

from util_decode_ref import lse_ref, mask_of, sample_ref, scaled
from util_gemm_ref import U32, check

pytestmark = pytest.mark.gpu

EOS = 2
SHAPES = ((3, 1003, torch.float32), (4, 1000, torch.float32), (2, 5003, torch.bfloat16), (1, 7, torch.float32))
# (temperature, suppress_eos, top_k, top_p): thresholds come from mic_warp_thresholds when top_k or top_p cut
OPTIONS = ((1.0, False, 0, 1.0), (0.7, False, 0, 1.0), (1.0, True, 0, 1.0), (0.7, True, 5, 1.0), (1.0, False, 50, 1.0), (0.7, True, 50, 0.9),
           (1.0, False, 0, 0.9))


def _logits(R, V, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * 3).to(dt)


def _key_words(keys):
    """uint32 [n][2] -> the int32 tensor ops.sample_rows_keyed takes (same bits)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(keys, np.uint32)).view(np.int32).copy())


def _thresholds(ops, xd, V, opt, dev):
    T, sup, k, p = opt
    if not (k or p < 1.0):
        return None, None
    R = xd.shape[0]
    thr = torch.empty(R, dtype=torch.float32, device=dev)
    lim = torch.empty(R, dtype=torch.int32, device=dev)
    ops.warp_thresholds(xd, xd.stride(0), V, thr, lim, R, temperature=T, suppress_eos=sup, eos_token_id=EOS, top_k=k, top_p=p)
    return thr, lim


def _n_r(V):
    return -(-V // 1024) + 2 + 6 + 15


def _logp_ref(x_row, drawn, T, sup, thr, lim):
    """(fp64 log p(drawn), bound) of one row of stored logits under the kernel's distribution: fp32(x / T), EOS and thresholds masked"""
    y = scaled(x_row, T, sup, EOS)
    if thr is not None:
        y = np.where(mask_of(y, thr, lim), y, -np.inf)
    lse, M, ls, e_ls = lse_ref(y, _n_r(y.size))
    lp = y[drawn] - lse
    return lp, e_ls + U32 * (abs(y[drawn] - M) + abs(lp))


@pytest.mark.parametrize("R,V,dt", SHAPES)
def test_one_draw_is_mic_sample_rows(dev, R, V, dt):
    from mic_amd import ops
    from oracle import generation_ref as G

    xd = _logits(R, V, dt, R * V).to(dev)
    key = G.prng_split(G.prng_key(R + V))[0]
    kd = _key_words([key]).to(dev)
    cut = 0
    for opt in OPTIONS:
        T, sup, k, p = opt
        thr, lim = _thresholds(ops, xd, V, opt, dev)
        want = torch.full((R,), -1, dtype=torch.int32, device=dev)
        got = torch.full((R,), -2, dtype=torch.int32, device=dev)
        kw = dict(temperature=T, suppress_eos=sup, eos_token_id=EOS, min_keep=thr, tie_limit=lim)
        ops.sample_rows(xd, xd.stride(0), V, key, want, R, **kw)
        ops.sample_rows_keyed(xd, xd.stride(0), V, kd, got, R, 1, **kw)
        assert torch.equal(got, want), (opt, got.tolist(), want.tolist())
        assert (got >= 0).all() and (got < V).all()
        if sup:
            assert (got != EOS).all()
        cut += thr is not None and bool(torch.isfinite(thr).any())
    assert cut >= 2 or V <= 50  # the threshold cases did cut something
    # a row pitch wider than V and a row base off the 16-byte grid: the scalar head and tail of the wide loads
    wide = torch.zeros((R, V + 11), dtype=dt, device=dev)
    view = wide[:, 3:3 + V]
    view.copy_(xd)
    want, got = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    ops.sample_rows(view, view.stride(0), V, key, want, R)
    ops.sample_rows_keyed(view, view.stride(0), V, kd, got, R, 1)
    assert torch.equal(got, want)
    ops.sample_rows_keyed(xd, xd.stride(0), V, kd, got, R, 1, forced_token=5)
    assert (got == 5).all()


@pytest.mark.parametrize("draws", [2, 3, 4])
@pytest.mark.parametrize("V,dt", [(1003, torch.float32), (1000, torch.float32), (5003, torch.bfloat16)])
def test_rows_of_draw_n_are_a_separate_call_with_key_n(dev, draws, V, dt):
    from mic_amd import ops
    from oracle import generation_ref as G

    images = 3
    R = images * draws
    x = _logits(R, V, dt, 7 * V + draws)
    xd = x.to(dev)
    keys = G.prng_split(G.prng_key(100 + draws), draws)
    kd = _key_words(keys).to(dev)
    decisive = total = 0
    for opt in ((1.0, False, 0, 1.0), (0.7, True, 0, 1.0), (0.7, True, 50, 0.9), (1.0, False, 5, 1.0)):
        T, sup, k, p = opt
        thr, lim = _thresholds(ops, xd, V, opt, dev)
        got = torch.empty(R, dtype=torch.int32, device=dev)
        ops.sample_rows_keyed(xd, xd.stride(0), V, kd, got, images, draws, temperature=T, suppress_eos=sup, eos_token_id=EOS, min_keep=thr, tie_limit=lim)
        got = got.cpu().numpy()
        for n in range(draws):
            sub = xd[n::draws].contiguous()
            t_n, l_n = (None, None) if thr is None else (thr[n::draws].contiguous(), lim[n::draws].contiguous())
            want = torch.empty(images, dtype=torch.int32, device=dev)
            ops.sample_rows(sub, sub.stride(0), V, keys[n], want, images, temperature=T, suppress_eos=sup, eos_token_id=EOS, min_keep=t_n, tie_limit=l_n)
            assert np.array_equal(got[n::draws], want.cpu().numpy()), (opt, n)
            ref, ok, info = sample_ref(x[n::draws].float().numpy().astype(np.float64), keys[n], T, suppress_eos=sup, eos=EOS,
                                       thr=None if thr is None else t_n.cpu().numpy(), lim=None if thr is None else l_n.cpu().numpy())
            for i in range(images):
                total += 1
                if ok[i]:
                    decisive += 1
                    assert got[n::draws][i] == ref[i], (opt, n, i, info[i])
        if not k and p == 1.0:  # different keys: the draws of one image are not copies of each other
            assert any(len(set(got[i * draws:(i + 1) * draws].tolist())) > 1 for i in range(images))
    assert decisive > 0.9 * total, (decisive, total)  # the fp64 comparison is not vacuous


@pytest.mark.parametrize("V,dt", [(1003, torch.float32), (5003, torch.bfloat16), (7, torch.float32)])
def test_log_probability_of_the_draw(dev, V, dt):
    from mic_amd import ops
    from oracle import generation_ref as G

    images, draws = 3, 2
    R = images * draws
    x = _logits(R, V, dt, 11 * V)
    xd = x.to(dev)
    x64 = x.float().numpy().astype(np.float64)
    kd = _key_words(G.prng_split(G.prng_key(9), draws)).to(dev)
    worst = 0.0
    for opt in ((1.0, False, 0, 1.0), (0.7, True, 0, 1.0), (0.7, True, 50, 0.9), (1.0, False, 5, 1.0)):
        T, sup, k, p = opt
        thr, lim = _thresholds(ops, xd, V, opt, dev)
        th, li = (None, None) if thr is None else (thr.cpu().numpy(), lim.cpu().numpy())
        kw = dict(temperature=T, suppress_eos=sup, eos_token_id=EOS, min_keep=thr, tie_limit=lim)
        fin = torch.zeros(R, dtype=torch.int32, device=dev)
        fin[1] = 1  # a finished row does not accumulate
        runs = []
        for _ in range(2):
            score = torch.full((R,), 0.25, dtype=torch.float32, device=dev)
            got = torch.empty(R, dtype=torch.int32, device=dev)
            ops.sample_rows_keyed(xd, xd.stride(0), V, kd, got, images, draws, finished=fin, score=score, **kw)
            runs.append((got.cpu().numpy(), score.cpu().numpy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1].tobytes() == runs[1][1].tobytes()  # the same bytes, the same bits
        got, score = runs[0]
        assert score[1] == np.float32(0.25)
        live = [r for r in range(R) if r != 1]
        ref = [_logp_ref(x64[r], int(got[r]), T, sup, None if th is None else th[r], None if li is None else li[r]) for r in live]
        lp = np.array([a for a, _ in ref])
        # score = fp32(0.25 + logp32): one more rounding of the sum
        bound = np.array([b for _, b in ref]) + U32 * np.abs(0.25 + lp)
        assert (lp <= 0).all() and np.isfinite(lp).all()
        worst = max(worst, check(score[live].astype(np.float64) - 0.25, lp, bound, f"log p of the draw V={V} {opt}"))
        # the draw itself is untouched by the score arguments, and without them nothing is written
        plain = torch.empty(R, dtype=torch.int32, device=dev)
        ops.sample_rows_keyed(xd, xd.stride(0), V, kd, plain, images, draws, **kw)
        assert np.array_equal(plain.cpu().numpy(), got)
        # no finished flags: every row accumulates
        score = torch.zeros(R, dtype=torch.float32, device=dev)
        ops.sample_rows_keyed(xd, xd.stride(0), V, kd, plain, images, draws, score=score, **kw)
        assert (score.cpu().numpy() <= 0).all() and score.cpu().numpy()[1] < 0
    # a forced token is a point mass: it adds 0
    score = torch.full((R,), -1.5, dtype=torch.float32, device=dev)
    got = torch.empty(R, dtype=torch.int32, device=dev)
    ops.sample_rows_keyed(xd, xd.stride(0), V, kd, got, images, draws, forced_token=4, finished=torch.zeros(R, dtype=torch.int32, device=dev), score=score)
    assert (got == 4).all() and (score == -1.5).all()
    print(f"[sample_keyed] V={V} {dt}: worst |logp - fp64| / bound {worst:.3g}")


def test_top_k_one_is_the_argmax_with_log_probability_zero(dev):
    """one survivor per row: no noise can change the draw, and log p = 0 exactly"""
    from mic_amd import ops
    from oracle import generation_ref as G

    images, draws, V = 2, 2, 1003
    R = images * draws
    x = _logits(R, V, torch.float32, 3)
    xd = x.to(dev)
    thr, lim = _thresholds(ops, xd, V, (1.0, False, 1, 1.0), dev)
    score = torch.zeros(R, dtype=torch.float32, device=dev)
    got = torch.empty(R, dtype=torch.int32, device=dev)
    ops.sample_rows_keyed(xd, xd.stride(0), V, _key_words(G.prng_split(G.prng_key(1), draws)).to(dev), got, images, draws, min_keep=thr,
                          tie_limit=lim, score=score)
    assert np.array_equal(got.cpu().numpy(), x.numpy().argmax(-1)) and (score == 0).all()


def test_bad_arguments_are_refused(dev):
    from mic_amd import ops
    from mic_amd._lib import MicError

    xd = torch.zeros((4, 16), dtype=torch.float32, device=dev)
    out = torch.empty(4, dtype=torch.int32, device=dev)
    keys = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    with pytest.raises(MicError):
        ops.sample_rows_keyed(xd, 8, 16, keys, out, 2, 2)  # ld < V
    with pytest.raises(MicError):
        ops.sample_rows_keyed(xd, 16, 16, keys, out, 2, 2, forced_token=16)
    with pytest.raises(MicError):
        ops.sample_rows_keyed(xd, 16, 16, keys[:1], out, 2, 2)  # one key for two draws
    with pytest.raises(MicError):
        ops.sample_rows_keyed(xd, 16, 16, keys, out, 2, 2, temperature=0.0)
    assert math.isfinite(float(xd.sum().item()))  # the device is fine after the refusals
