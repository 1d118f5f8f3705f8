"""Shared by the gradient-clipping tests (tests/test_clip_gpu.py, tests/test_clip_ddp_gpu.py): the derived error bound of the sum of
squares, the oracle's micro-batch gradients, and the assertions made after a clipped optimizer step."""
import math

import numpy as np
import torch

from util_small import batch

B, T = 2, 12
B1, B2 = 0.9, 0.999
EPS24 = 2.0 ** -24
# (1 - b1), (1 - b2) as the AdamW kernels hold them: formed in double, rounded once to fp32 (include/mic_hip.h)
OMB1, OMB2 = float(np.float32(1.0 - B1)), float(np.float32(1.0 - B2))


def as_batch(shard):
    px, labels, mask, dec_in = shard
    return {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}


def sumsq_rel_bound(n, slots):
    """Relative error bound of mic_grad_sumsq's result (its slots added exactly) against the exact sum of the squares of the same fp32
    values.  All terms are non-negative, so the relative error of the sum is at most that of its worst term: each square is rounded
    once, and the longest chain of fp32 additions a term passes through is 4 * ceil(n/4 / threads_in_grid) + 8 (per-thread
    accumulation, the 6-stage wave butterfly, the 2-stage combination of the four waves) — (chain + 2) * 2^-24 to first order, the 2
    covering the square's rounding and the second-order terms.  The tests assert twice this."""
    threads = slots * 256
    chain = 4 * math.ceil((n // 4) / threads) + 8
    return (chain + 2) * EPS24


_ORACLE = {}


def oracle(rc, p, seed):
    """(shard, loss, grads) of the oracle on the micro-batch of `seed` at the INITIAL parameters: computed once, shared, never modified"""
    from oracle import train_ref

    if seed not in _ORACLE:
        sh = batch(rc, B, T, seed=seed, ragged=True)
        l, g = train_ref.loss_and_grads(rc, p, *sh)
        _ORACLE[seed] = (sh, l.item(), g)
    return _ORACLE[seed]


def norm64(grads):
    """global L2 norm of a {leaf: array} gradient in fp64"""
    return math.sqrt(sum(float((torch.as_tensor(np.asarray(g)).double() ** 2).sum()) for g in grads.values()))


def clip_factor(norm, c):
    """optax.clip_by_global_norm: the factor on the gradient (strict trigger)"""
    return 1.0 if norm < c else c / norm


def stored_gradient(store, with_acc):
    """the summed gradient the optimizer step consumed, per leaf in the reference layout (padding excluded): `grad`, plus `acc` with one
    IEEE fp32 add per element where AdamW read g + acc"""
    g = store.export_flat("grad")
    if with_acc:
        a = store.export_flat("acc")
        g = {k: g[k] + a[k] for k in g}
    assert all(v.dtype == np.float32 for v in g.values())
    return g


def trainer_chain_bound(tr):
    """`sumsq_rel_bound` of the launches this Trainer's norm is made of (the worst of them: the terms are non-negative)"""
    from mic_amd import ops

    pieces = tr.buckets if tr.reducer.on_ready is not None else [(0, tr.model.store.numel)]
    return max(sumsq_rel_bound(e - b, ops.grad_sumsq_slots(e - b)) for (b, e) in pieces)


def assert_tight(tr, out, c, with_acc, m_prev=None, v_prev=None, tag=""):
    """The mode-independent assertions after an optimizer step with clipping, all against the model's OWN stored gradient:
    (1) grad_norm = gscale * the fp64 norm of that gradient, at the kernel's bound: the norm is the square root of the sum (half its
        relative error) rounded once to fp32 (2^-24), together below `sumsq_rel_bound`; asserted at twice that.
    (2) m / (1 - b1) = coef * g per leaf to 4 * 2^-24 of the leaf's scale, coef rebuilt from the read-back norm by the clip formula
        (roundings: the norm and the coefficient to fp32, g * coef, (1 - b1) * that; m starts at 0, so b1 * m adds nothing).
    (3) v / (1 - b2) = (coef * g)^2 at 8 * 2^-24 (twice the three roundings of coef * g, and the two products).
    With m_prev / v_prev (a later step): m = b1 * m_prev + (1 - b1) * coef * g at 5 * 2^-24 of scale(b1 m_prev) + scale((1 - b1) coef g)
    (the four roundings of (2), the rounding of b1 * m_prev or of the other product under contraction, and that of the final sum), v
    likewise at 9 * 2^-24.  Returns (norm read back, coef)."""
    st = tr.model.store
    gs = float(np.float32(tr._gscale))  # (the kernels receive grad_scale as a float)
    g = stored_gradient(st, with_acc)
    ref = gs * norm64(g)
    got = float(out["grad_norm"])
    bound = 2.0 * trainer_chain_bound(tr)
    rel = abs(got - ref) / ref
    print(f"[clip{tag}] grad_norm {got!r} vs fp64 of the stored gradient {ref!r}: relative {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound, (got, ref, rel, bound)
    coef = gs if got < c else gs * c / got
    dev_coef = float(tr._clip_out[1])
    assert abs(dev_coef - coef) <= 2.0 ** -23 * coef, (dev_coef, coef)
    m, v = st.export_flat("m"), st.export_flat("v")
    worst_m = worst_v = 0.0
    for k in g:
        cg = coef * torch.from_numpy(g[k]).double()
        mk, vk = torch.from_numpy(m[k]).double(), torch.from_numpy(v[k]).double()
        if m_prev is None:
            want_m, sc_m, tol_m = cg, cg.abs().max().item(), 4 * EPS24
            want_v, sc_v, tol_v = cg * cg, (cg * cg).max().item(), 8 * EPS24
            mk, vk = mk / OMB1, vk / OMB2
        else:
            pm, pv = float(np.float32(B1)) * torch.from_numpy(m_prev[k]).double(), float(np.float32(B2)) * torch.from_numpy(v_prev[k]).double()
            want_m, sc_m, tol_m = pm + OMB1 * cg, pm.abs().max().item() + OMB1 * cg.abs().max().item(), 5 * EPS24
            want_v, sc_v, tol_v = pv + OMB2 * cg * cg, pv.max().item() + OMB2 * (cg * cg).max().item(), 9 * EPS24
        if sc_m > 0:
            e = (mk - want_m).abs().max().item() / sc_m
            worst_m = max(worst_m, e / tol_m)
            assert e <= tol_m, ("m", k, e, tol_m)
        if sc_v > 0:
            e = (vk - want_v).abs().max().item() / sc_v
            worst_v = max(worst_v, e / tol_v)
            assert e <= tol_v, ("v", k, e, tol_v)
    print(f"[clip{tag}] coef {coef!r}; worst leaf error as a share of its bound: m {worst_m:.3f}, v {worst_v:.3f}")
    return got, coef


def assert_oracle(tr, out, p, oracle_grads, c, fp32, lr=1e-3, wd=0.01, tag=""):
    """against the oracle: grad_norm within 5e-4 (fp32) / 8e-2 (bf16) relative of the norm of the oracle's mean gradient (the
    per-tensor gradient bounds of tests/test_accumulate_gpu.py, used as caps), and — fp32 — the weights within 1e-4 of the oracle's
    AdamW step on min(1, c / norm) * that gradient.  Returns the measured relative distance of the norm."""
    from mic_amd.params import flatten_tree
    from oracle import train_ref

    n_ref = norm64(oracle_grads)
    got = float(out["grad_norm"])
    cap = 5e-4 if fp32 else 8e-2
    rel = abs(got - n_ref) / n_ref
    print(f"[clip{tag}] grad_norm {got:.6f} vs oracle {n_ref:.6f}: relative {rel:.3e} (cap {cap:.0e}, a quarter of it {cap / 4:.1e})")
    assert rel <= cap, (got, n_ref, rel)
    if fp32:
        f = clip_factor(n_ref, c)
        now = flatten_tree(tr.model.params)
        for k in p:
            newp, _, _ = train_ref.adamw_update(p[k], f * oracle_grads[k], torch.zeros_like(p[k]), torch.zeros_like(p[k]), 0, lr, wd=wd)
            d = (torch.from_numpy(now[k]).reshape(newp.shape) - newp).abs().max().item()
            assert d < 1e-4, (k, d)
    return rel
