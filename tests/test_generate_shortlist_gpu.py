"""generate(allowed_token_ids=A): the LM head and the top-k over a shortlist of the vocabulary.

The contract: the call returns what the same call returns on a model whose final_logits_bias is -inf outside A.  That reference
needs no new oracle code: the oracle's params are a dict, the tests below set final_logits_bias to -1e30 outside A (not -inf: no
inf - inf anywhere) and call the oracle as tests/test_generate_gpu.py does.

Kernel level: the mapped top-k entry points against the unmapped ones composed with the map (bitwise), the shortlist head GEMM
against the fp64 product of the gathered operands.  Model level, float32: ids and step counts exact, scores to 1e-4 (the bounds of
test_beam_ids_exact).  A randomly initialised reduced model mostly repeats the token it was fed, so A is built per case from a
random ~300-id set MINUS every token the full-vocabulary oracle emitted (plus EOS and the forced ids): the masked oracle then has to
answer differently, which the tests assert — an ignored argument cannot pass.  bfloat16: emitted ids lie in A, and one decoder
step's shortlist logits pick the candidates the gathered full-vocabulary logits pick wherever those are decisive."""
import numpy as np
import pytest
import torch

from test_generate_gpu import _oracle_gen
from util_small import SEED, batch, make_pair

pytestmark = pytest.mark.gpu

B = 3


# ------------------------------------------------------------------------------------------------ helpers
def _masked(rc, p, A):
    """the oracle's params with final_logits_bias = -1e30 outside A, unchanged inside"""
    q = dict(p)
    flb = p["final_logits_bias"].clone()
    out = torch.ones(rc.vocab_size, dtype=torch.bool)
    out[torch.as_tensor(np.asarray(A), dtype=torch.long)] = False
    flb[0, out] = -1e30
    q["final_logits_bias"] = flb
    return q


def _build_A(rc, emitted, extra, seed, n=300):
    """a random n-id set without any token of `emitted`, plus `extra` (EOS, forced ids): sorted unique int32"""
    rng = np.random.default_rng(seed)
    base = rng.choice(np.arange(4, rc.vocab_size), size=n, replace=False)
    A = set(base.tolist()) - set(np.asarray(emitted).reshape(-1).tolist())
    A |= set(int(e) for e in extra if e is not None)
    return np.array(sorted(A), dtype=np.int32)


def _seq(ref, kw):
    return ref.sequences if kw.get("num_beams", 1) > 1 else ref


def _extra(rc, kw):
    ids = [rc.eos_token_id, kw.get("forced_eos_token_id", 2)]
    for name in ("forced_bos_token_id",):
        v = kw.get(name)
        ids.extend(v if isinstance(v, (list, tuple)) else [v])
    return ids


def _case_A(rc, p, px, kw, seed):
    """(A, full-vocabulary oracle result, masked oracle result) of one single-language case"""
    full = _oracle_gen(rc, p, px, px.shape[0], **kw)
    A = _build_A(rc, _seq(full, kw), _extra(rc, kw), seed)
    ref = _oracle_gen(rc, _masked(rc, p, A), px, px.shape[0], **kw)
    allowed = np.concatenate([A, [rc.pad_token_id, kw.get("decoder_start_token_id", 2)]])
    assert np.isin(_seq(ref, kw), allowed).all()  # the reference itself: nothing outside A but PAD and the start token
    return A, full, ref


def _check(out, ref, kw, what=""):
    beam = kw.get("num_beams", 1) > 1
    assert np.array_equal(out.sequences.cpu().numpy(), _seq(ref, kw)), (what, kw, out.sequences, _seq(ref, kw))
    if beam:
        assert out["steps"] == ref.steps, (what, out["steps"], ref.steps)
        assert np.isfinite(ref.scores).all()
        assert np.allclose(out.scores.cpu().numpy(), ref.scores, rtol=1e-4, atol=1e-4), (what, out.scores, ref.scores)


def _differs(full, ref, kw) -> float:
    return float((_seq(full, kw) != _seq(ref, kw)).mean())


@pytest.fixture(scope="module")
def fp32(dev):
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    px, *_ = batch(rc, B, 12, seed=21)
    yield rc, p, model, px
    model.release_decode_plans()


# ------------------------------------------------------------------------------------------------ kernel level
def _grid_logits(dev, R, Vs, ld, seed):
    """bf16 logits [R][ld] on a coarse grid (ties within and across 64-column granules) written by the head-form GEMM together with
    its per-granule softmax partials: row r of x is the unit vector e_r, so logits[r][c] = w[c][r] exactly"""
    from mic_amd import ops

    K = 256
    g = torch.Generator().manual_seed(seed)
    vals = torch.randint(0, 6, (R, Vs), generator=g).float() / 4 - 1.0
    vals[1] = 0.25                       # a row of one value: every granule ties
    vals[2, 3] = 2.0                     # the column the tests treat as EOS leads row 2 (and is its granule's maximum)
    vals[3, Vs - 1] = 3.0                # the last valid column leads row 3
    x = torch.zeros(128, K, dtype=torch.bfloat16)
    x[torch.arange(R), torch.arange(R)] = 1.0
    w = torch.zeros(ld, K, dtype=torch.bfloat16)
    w[:Vs, :R] = vals.t().to(torch.bfloat16)
    logits = torch.full((128, ld), 9.0, dtype=torch.bfloat16, device=dev)   # whatever lies behind column Vs must not win
    stat = torch.full((128, ld // 64, 2), float("nan"), device=dev)
    ops.gemm(x.to(dev), w.to(dev), logits, R, ld, K, bias=torch.zeros(ld, device=dev), rowstat=stat, rowstat_nvalid=Vs)
    logits[:, Vs:] = 9.0                 # the GEMM wrote its padding columns (zeros): make them attractive
    torch.cuda.synchronize()
    assert torch.equal(logits[:R, :Vs].float().cpu(), vals)
    return logits, stat


def _map(Vs, seed, V=1003):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(V, size=Vs, replace=False)).astype(np.int32)


def _bits(t):
    return t.view(torch.int32)


_VARIANTS = [dict(), dict(bias=True), dict(suppress_eos=True), dict(bias=True, suppress_eos=True)]


@pytest.mark.parametrize("Vs", [67, 128, 129])
def test_mapped_streaming_topk_is_the_unmapped_one_composed_with_the_map(dev, Vs):
    from mic_amd import _lib as L
    from mic_amd import ops

    R, ld = 5, -(-Vs // 128) * 128
    lg16, _ = _grid_logits(dev, R, Vs, ld, seed=Vs)
    tmap = _map(Vs, Vs)
    tmap_d = torch.from_numpy(tmap).to(dev)
    rb = torch.linspace(-3.0, 0.5, R).to(dev)
    for logits in (lg16, lg16.float()):
        for k, raw in ((1, True), (8, False), (20, False), (64, False)):
            for var in _VARIANTS + [dict(forced=0), dict(forced=Vs - 1, bias=True), dict(forced=min(5, Vs - 1))]:
                kw = dict(forced_token=var.get("forced", -1), suppress_eos=var.get("suppress_eos", False), eos_token_id=3, raw_logits=raw,
                          row_bias=rb if var.get("bias") else None)
                v0, i0 = torch.full((R, k), 7.0, device=dev), torch.full((R, k), -7, dtype=torch.int32, device=dev)
                v1, i1 = torch.full((R, k), 8.0, device=dev), torch.full((R, k), -8, dtype=torch.int32, device=dev)
                v2, i2 = torch.full((R, k), 9.0, device=dev), torch.full((R, k), -9, dtype=torch.int32, device=dev)
                ops.row_lse_topk(logits, ld, Vs, k, v0, i0, R, **kw)
                ops.row_lse_topk(logits, ld, Vs, k, v1, i1, R, token_map=tmap_d, **kw)
                L.check(L.lib().mic_row_lse_topk_mapped(ops._dt(logits), R, Vs, ops._p(logits), ld, k, kw["forced_token"], int(kw["suppress_eos"]), 3,
                                                        int(raw), ops._p(kw["row_bias"]), ops._p(v2), ops._p(i2), None, ops._stream()), "null map")
                torch.cuda.synchronize()
                what = (str(logits.dtype), k, var)
                c0 = i0.cpu().numpy()
                assert (c0 >= 0).all() and (c0 < Vs).all(), what          # columns behind Vs never win
                assert torch.equal(_bits(v1), _bits(v0)), what             # values bitwise (-inf included)
                assert np.array_equal(i1.cpu().numpy(), tmap[c0]), what    # ids = map o columns
                assert torch.equal(_bits(v2), _bits(v0)) and torch.equal(i2, i0), what   # a null map is the old entry point
                if var.get("suppress_eos") and not raw:
                    assert not (c0[torch.isfinite(v0).cpu().numpy()] == 3).any(), what
                if "forced" not in var and not var.get("suppress_eos") and k == 1:
                    assert c0[2, 0] == 3 and c0[3, 0] == Vs - 1 and c0[1, 0] == 0, what   # the planted leaders, first index among ties


@pytest.mark.parametrize("Vs", [67, 128, 129])
def test_mapped_granule_topk_is_the_unmapped_one_composed_with_the_map(dev, Vs):
    from mic_amd import _lib as L
    from mic_amd import ops

    R, ld = 5, -(-Vs // 128) * 128
    logits, stat = _grid_logits(dev, R, Vs, ld, seed=1000 + Vs)
    tmap = _map(Vs, 1000 + Vs)
    tmap_d = torch.from_numpy(tmap).to(dev)
    rb = torch.linspace(-3.0, 0.5, R).to(dev)
    for k in (2, 8, 16):
        for raw in (False, True):
            for var in _VARIANTS:
                kw = dict(suppress_eos=var.get("suppress_eos", False), eos_token_id=3, raw_logits=raw, row_bias=rb if var.get("bias") else None)
                v0, i0 = torch.full((R, k), 7.0, device=dev), torch.full((R, k), -7, dtype=torch.int32, device=dev)
                v1, i1 = torch.full((R, k), 8.0, device=dev), torch.full((R, k), -8, dtype=torch.int32, device=dev)
                v2, i2 = torch.full((R, k), 9.0, device=dev), torch.full((R, k), -9, dtype=torch.int32, device=dev)
                vs, is_ = torch.full((R, k), 6.0, device=dev), torch.full((R, k), -6, dtype=torch.int32, device=dev)
                ops.row_topk_tiles(logits, ld, Vs, stat, k, v0, i0, R, **kw)
                ops.row_topk_tiles(logits, ld, Vs, stat, k, v1, i1, R, token_map=tmap_d, **kw)
                L.check(L.lib().mic_row_topk_tiles_mapped(ops._dt(logits), R, Vs, ops._p(logits), ld, ops._p(stat), stat.stride(0) // 2, k,
                                                          int(kw["suppress_eos"]), 3, int(raw), ops._p(kw["row_bias"]), ops._p(v2), ops._p(i2), None,
                                                          ops._stream()), "null map")
                ops.row_lse_topk(logits, ld, Vs, k, vs, is_, R, token_map=tmap_d, **kw)   # the streaming kernel on the same logits
                torch.cuda.synchronize()
                what = (k, raw, var)
                c0 = i0.cpu().numpy()
                assert (c0 >= 0).all() and (c0 < Vs).all(), what
                assert torch.equal(_bits(v1), _bits(v0)), what
                assert np.array_equal(i1.cpu().numpy(), tmap[c0]), what
                assert torch.equal(_bits(v2), _bits(v0)) and torch.equal(i2, i0), what
                assert torch.equal(i1, is_), what   # both kernels name the same tokens in the same order


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shortlist_head_against_the_fp64_product_of_the_gathered_operands(dev, dtype):
    """Engine.head_logits(shortlist=...) for R in {5, 130} rows and Ns in {67, 128, 300} ids: the logits under the bound the GEMM
    conformance suite applies to this epilogue (util_gemm_ref: fp32 accumulation over K, bias, one rounding to the stored type); the
    top-k over them never names a padding column; bfloat16: the granule kernel on the GEMM's partials names the streaming kernel's ids"""
    import util_gemm_ref as GR
    from mic_amd import ops

    rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    eng, st = model.engine, model.store
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    flb = torch.randn(st.Vpad, generator=torch.Generator().manual_seed(3)) * 0.5   # a bias that matters
    st.f32("flb").copy_(flb.to(dev))
    model.invalidate_params_cache()
    E = st.w("shared").float().cpu().double().numpy()
    for Ns in (67, 128, 300):
        ids = _map(Ns, Ns, st.V)
        sl = model._shortlist(ids)
        sl.refresh()
        assert sl.Ns == Ns and sl.Ns_pad == -(-Ns // 128) * 128 and tuple(sl.E.shape) == (sl.Ns_pad, st.d) and sl.E.dtype == dtype
        assert np.array_equal(sl.map.cpu().numpy(), ids) and sl.map.dtype == torch.int32 and sl.bias.dtype == torch.float32
        assert torch.equal(sl.E[:Ns].cpu(), st.w("shared")[torch.from_numpy(ids).long().to(dev)].cpu()) and not bool(sl.E[Ns:].any())
        assert torch.equal(sl.bias[:Ns].cpu(), flb[torch.from_numpy(ids).long()]) and not bool(sl.bias[Ns:].any())
        for R in (5, 130):
            g = torch.Generator().manual_seed(R + Ns)
            hf = torch.zeros(256, st.d, dtype=dtype, device=dev)
            hf[:R] = torch.randn(R, st.d, generator=g).to(dtype).to(dev)
            full = eng.head_logits(hf, R, name="t.logits").clone()
            logits, stat = eng.head_logits(hf, R, name="t.logits", stats=True, shortlist=sl)
            torch.cuda.synchronize()
            assert tuple(logits.shape)[1] == sl.Ns_pad and (stat is None) == (dtype == torch.float32)
            ref = GR.gemm_ref(hf[:R].float().cpu().double().numpy(), E[ids].T, bias=flb[torch.from_numpy(ids).long()].double().numpy(), c_dtype=name)
            GR.check(logits[:R, :Ns].float().cpu().numpy(), ref["C"], ref["bound_C"], f"shortlist head {name} R={R} Ns={Ns}")
            assert torch.equal(eng.head_logits(hf, R, name="t.logits"), full)   # the full-vocabulary buffers are their own
            for k in (2, 16):
                rb = torch.linspace(-1.0, 0.0, R).to(dev)
                v1, i1 = torch.empty((R, k), device=dev), torch.empty((R, k), dtype=torch.int32, device=dev)
                ops.row_lse_topk(logits, logits.stride(0), Ns, k, v1, i1, R, eos_token_id=0, row_bias=rb, token_map=sl.map)
                torch.cuda.synchronize()
                got = i1.cpu().numpy()
                assert np.isin(got, ids).all()   # padding columns (and anything else off the list) never win
                lp = logits[:R, :Ns].float().cpu().double()
                lp = (lp - torch.logsumexp(lp, -1, keepdim=True)).numpy() + rb.cpu().double().numpy()[:, None]
                kth = np.sort(lp, axis=1)[:, -k]
                col = np.searchsorted(ids, got)
                assert (np.take_along_axis(lp, col, 1) >= kth[:, None] - 1e-4).all() and np.allclose(v1.cpu().numpy(), np.take_along_axis(lp, col, 1), atol=1e-4)
                assert all(len(set(r)) == k for r in got.tolist())
                if stat is not None:
                    v2, i2 = torch.empty((R, k), device=dev), torch.empty((R, k), dtype=torch.int32, device=dev)
                    ops.row_topk_tiles(logits, logits.stride(0), Ns, stat, k, v2, i2, R, eos_token_id=0, row_bias=rb, token_map=sl.map)
                    torch.cuda.synchronize()
                    assert torch.equal(i2, i1), (R, Ns, k)
                    assert (v2 - v1).abs().max().item() < 2e-5


# ------------------------------------------------------------------------------------------------ model level, float32
@pytest.mark.parametrize("kw,must_differ", [(dict(max_length=10), False),   # (the default start token is EOS: greedy stops at once, with or without A)
                                            (dict(max_length=10, min_length=4), True),
                                            (dict(max_length=12, forced_bos_token_id=996), False),   # repeats 996: checks the forced column
                                            (dict(max_length=9, decoder_start_token_id=999, forced_eos_token_id=None), True)])
def test_greedy_equals_the_oracle_with_the_masked_bias(fp32, kw, must_differ):
    rc, p, model, px = fp32
    kw = dict(kw, num_beams=1)
    A, full, ref = _case_A(rc, p, px, kw, seed=len(str(kw)))
    print(f"greedy {kw}: len(A) = {len(A)}, masked oracle differs from the full-vocabulary one at {_differs(full, ref, kw):.2f} of the positions")
    if must_differ:
        assert _differs(full, ref, kw) > 0.5
    out = model.generate(px.numpy(), allowed_token_ids=A, **kw)
    _check(out, ref, kw)
    shuffled = np.random.default_rng(0).permutation(np.concatenate([A, A[:7]])).tolist()   # order and duplicates do not matter
    _check(model.generate(px.numpy(), allowed_token_ids=shuffled, **kw), ref, kw, "shuffled list")


@pytest.mark.parametrize("kw,must_differ", [(dict(max_length=10, num_beams=4, forced_bos_token_id=996), False),
                                            (dict(max_length=9, num_beams=5, decoder_start_token_id=999), True),
                                            (dict(max_length=8, num_beams=12, decoder_start_token_id=999), True),   # streaming 32-wide build
                                            (dict(max_length=6, num_beams=32, length_penalty=1.2, decoder_start_token_id=999), True)])
def test_beam_equals_the_oracle_with_the_masked_bias(fp32, kw, must_differ):
    rc, p, model, px = fp32
    A, full, ref = _case_A(rc, p, px, kw, seed=len(str(kw)))
    print(f"beam {kw}: len(A) = {len(A)}, masked oracle differs from the full-vocabulary one at {_differs(full, ref, kw):.2f} of the positions")
    if must_differ:
        assert _differs(full, ref, kw) > 0.5
    out = model.generate(px.numpy(), allowed_token_ids=torch.from_numpy(A), **kw)
    assert tuple(out.sequences.shape) == (B, kw["max_length"]) and tuple(out.scores.shape) == (B,)
    _check(out, ref, kw)


def test_beam_early_finish_with_eos_on_the_list(dev):
    """EOS pushed up through final_logits_bias (+6.0) and kept in A: beams finish early — the finished-merge, the stop test and the
    'no-op after stop' launches with the shortlist head, early_stopping on and off"""
    from mic_amd.params import unflatten_tree

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    p = dict(p)
    flb = p["final_logits_bias"].clone()
    flb[0, rc.eos_token_id] = 6.0
    p["final_logits_bias"] = flb
    model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
    px, *_ = batch(rc, 4, 12, seed=23)
    saw_eos = False
    for kw in (dict(max_length=12, num_beams=4, decoder_start_token_id=999), dict(max_length=12, num_beams=3, early_stopping=False, decoder_start_token_id=999)):
        A, full, ref = _case_A(rc, p, px, kw, seed=kw["num_beams"])
        print(f"early finish {kw}: steps {ref.steps} (full vocabulary {full.steps}), differs at {_differs(full, ref, kw):.2f}")
        assert rc.eos_token_id in A
        out = model.generate(px.numpy(), allowed_token_ids=A, **kw)
        _check(out, ref, kw)
        saw_eos = saw_eos or bool((ref.sequences[:, 1:-1] == rc.eos_token_id).any())
    assert saw_eos   # hypotheses did finish before the forced EOS


@pytest.mark.parametrize("kw", [dict(decoder_start_token_id=[999, 998, 997], num_beams=1, max_length=10, forced_eos_token_id=None),
                                dict(forced_bos_token_id=[996, 995, 994], num_beams=1, max_length=10),
                                dict(decoder_start_token_id=[999, 998, 997], num_beams=4, max_length=10),
                                dict(forced_bos_token_id=[996, 995, 994], num_beams=4, max_length=10)])
def test_grouped_languages_share_one_shortlist(fp32, kw):
    """G = 3 languages in one call with one A: equal to the masked oracle per language, and bitwise equal to three separate product
    calls with the same A"""
    rc, p, model, px = fp32
    G = 3
    calls = [{k: (v[g] if isinstance(v, list) else v) for k, v in kw.items()} for g in range(G)]
    fulls = [_oracle_gen(rc, p, px, B, **one) for one in calls]
    A = _build_A(rc, np.concatenate([_seq(f, kw).reshape(-1) for f in fulls]), _extra(rc, kw), seed=7 + kw["num_beams"])
    pm = _masked(rc, p, A)
    out = model.generate(px.numpy(), allowed_token_ids=A, **kw)
    assert tuple(out.sequences.shape) == (G, B, kw["max_length"])
    beam = kw["num_beams"] > 1
    changed = []
    for g, one in enumerate(calls):
        ref = _oracle_gen(rc, pm, px, B, **one)
        changed.append(_differs(fulls[g], ref, one))
        assert np.array_equal(out.sequences[g].cpu().numpy(), _seq(ref, one)), (g, one)
        if beam:
            assert out["steps"][g] == ref.steps and np.allclose(out.scores[g].cpu().numpy(), ref.scores, rtol=1e-4, atol=1e-4), g
        single = model.generate(px.numpy(), allowed_token_ids=A, **one)
        assert torch.equal(single.sequences, out.sequences[g]), g
        if beam:
            assert torch.equal(single.scores, out.scores[g]) and single["steps"] == out["steps"][g], g
    print(f"grouped {kw}: masked oracle differs from the full-vocabulary one at {changed} of the positions per language")
    if "decoder_start_token_id" in kw:
        assert min(changed) > 0.5


def test_generate_languages_passes_the_shortlist_on(fp32):
    from mic_amd.evaluation import generate_languages, vocabulary_shortlist

    rc, p, model, px = fp32
    langs = {"en_XX": 996, "fr_XX": 995}
    g = np.random.default_rng(5)
    captions = [g.integers(4, 900, size=(6, 12)), g.integers(4, 900, size=(3, 9))]
    A = vocabulary_shortlist(captions, always=[rc.eos_token_id, *langs.values()])
    got = generate_languages(model, px.numpy(), langs, max_length=8, num_beams=4, allowed_token_ids=A)
    pm = _masked(rc, p, A)
    for lang, tok in langs.items():
        ref = _oracle_gen(rc, pm, px, B, num_beams=4, max_length=8, forced_bos_token_id=tok)
        assert np.array_equal(got[lang], ref.sequences), lang


def test_graph_replay_a_second_set_and_new_weights(dev, monkeypatch):
    """MIC_DECODE_GRAPHS=1: call 1 of a plan is eager, call 2 captures the steps (shortlist pointers, column count, EOS column baked
    in) and replays, call 3 only replays — all equal to the masked oracle.  A second set of the same length gets a plan and a result
    of its own, and after the weights are replaced the first plan's captured steps read the re-gathered rows."""
    from mic_amd.params import unflatten_tree
    from oracle import model_ref as M

    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    p2 = M.init_params(rc, seed=SEED + 1, perturb_ln=True)
    for kw in (dict(max_length=12, num_beams=4, decoder_start_token_id=999), dict(max_length=14, num_beams=1, decoder_start_token_id=999)):
        model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
        model.release_decode_plans()
        px, *_ = batch(rc, B, 12, seed=31)
        A, full, ref = _case_A(rc, p, px, kw, seed=11)
        assert _differs(full, ref, kw) > 0.5
        for call, seed in enumerate((31, 32, 33)):
            px, *_ = batch(rc, B, 12, seed=seed)
            ref = _oracle_gen(rc, _masked(rc, p, A), px, B, **kw)
            out = model.generate(px.numpy(), allowed_token_ids=A, **kw)
            _check(out, ref, kw, f"call {call}")
            plan = next(iter(model._decode_plans.values()))
            assert len(model._decode_plans) == 1 and plan.calls == call + 1 and plan.shortlist is not None
            if call >= 1:
                assert len(plan.graphs) > 0 and 1 not in plan.graphs
        # a second set of the same length: other ids, its own plan, its own result
        other = _build_A(rc, np.concatenate([_seq(full, kw).reshape(-1), A]), [], seed=12, n=700)
        A2 = np.sort(np.concatenate([other[: len(A) - 1], [rc.eos_token_id]])).astype(np.int32)
        assert len(A2) == len(A) and not np.array_equal(A2, A)
        ref2 = _oracle_gen(rc, _masked(rc, p, A2), px, B, **kw)
        assert not np.array_equal(_seq(ref2, kw), _seq(ref, kw))
        for call in range(2):
            _check(model.generate(px.numpy(), allowed_token_ids=A2, **kw), ref2, kw, f"second set, call {call}")
        assert len(model._decode_plans) == 2
        _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref, kw, "first set again")
        # new weights: the same plan (its graphs are replayed), the gathered rows follow
        model.params = unflatten_tree({k: v.numpy() for k, v in p2.items()})
        ref3 = _oracle_gen(rc, _masked(rc, p2, A), px, B, **kw)
        assert not np.array_equal(_seq(ref3, kw), _seq(ref, kw))
        n_graphs = len(plan.graphs)
        _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref3, kw, "new weights")
        assert len(plan.graphs) >= n_graphs > 0 and next(iter(model._decode_plans.values())) is not None
        monkeypatch.setenv("MIC_DECODE_GRAPHS", "0")
        _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref3, kw, "new weights, eager")
        monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    model.release_decode_plans()


def test_the_gathered_rows_follow_a_train_step(dev):
    """a train step between two generate calls: the shortlist is re-gathered in place (same tensors, new values)"""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    px, labels, mask, dec_in = batch(rc, B, 12, seed=41)
    kw = dict(max_length=8, num_beams=4, decoder_start_token_id=999)
    A, full, ref = _case_A(rc, p, px, kw, seed=13)
    _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref, kw)
    sl = next(iter(model._shortlists.values()))
    ptr, before = sl.E.data_ptr(), sl.E.clone()
    tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, 1e-3))
    tr.train_step({"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()})
    p2 = {k: torch.from_numpy(np.asarray(v)) for k, v in flatten_tree(model.params).items()}
    ref2 = _oracle_gen(rc, _masked(rc, p2, A), px, B, **kw)
    _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref2, kw, "after a train step")
    assert next(iter(model._shortlists.values())) is sl and sl.E.data_ptr() == ptr and not torch.equal(sl.E, before)


def test_plain_generate_around_shortlist_calls_is_unchanged(fp32):
    rc, p, model, px = fp32
    for kw in (dict(max_length=10, num_beams=4, decoder_start_token_id=999), dict(max_length=10, num_beams=1, decoder_start_token_id=999)):
        A, full, ref = _case_A(rc, p, px, kw, seed=17)
        _check(model.generate(px.numpy(), **kw), full, kw, "plain before")
        _check(model.generate(px.numpy(), allowed_token_ids=A, **kw), ref, kw)
        _check(model.generate(px.numpy(), **kw), full, kw, "plain after")
        _check(model.generate(px.numpy(), allowed_token_ids=None, **kw), full, kw, "None is the plain call")
    # the shortlists are cached per distinct set, a few at most
    from mic_amd.generation_clip_vision_utils import _MAX_SHORTLISTS

    n = len(model._shortlists)
    model.generate(px.numpy(), allowed_token_ids=A, **kw)
    assert len(model._shortlists) == n <= _MAX_SHORTLISTS
    for i in range(_MAX_SHORTLISTS + 1):
        model.generate(px.numpy(), allowed_token_ids=np.concatenate([A, [3 + i]]), max_length=4, num_beams=1)
    assert len(model._shortlists) == _MAX_SHORTLISTS


def test_errors_through_generate(fp32):
    rc, p, model, px = fp32
    eos = rc.eos_token_id
    ok = list(range(100, 140)) + [eos]
    x = px.numpy()
    for bad in ([], [1.5, 2.0], np.array([[eos, 5]]), [eos, rc.vocab_size], [-1, eos], 7):
        with pytest.raises(ValueError, match="allowed_token_ids"):
            model.generate(x, allowed_token_ids=bad, max_length=5, num_beams=1)
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(x, allowed_token_ids=ok[:-1], max_length=5, num_beams=1)
    with pytest.raises(ValueError, match="forced_bos_token_id"):
        model.generate(x, allowed_token_ids=ok, forced_bos_token_id=996, max_length=5, num_beams=1)
    with pytest.raises(ValueError, match="forced_eos_token_id"):
        model.generate(x, allowed_token_ids=ok, forced_eos_token_id=3, max_length=5, num_beams=1)
    with pytest.raises(ValueError, match="language id 995"):
        model.generate(x, allowed_token_ids=ok + [996], forced_bos_token_id=[996, 995], max_length=5, num_beams=4)
    with pytest.raises(ValueError, match="num_beams=32"):
        model.generate(x, allowed_token_ids=ok, max_length=5, num_beams=32)
    with pytest.raises(NotImplementedError, match="allowed_token_ids"):
        model.generate(x, allowed_token_ids=ok, do_sample=True, num_beams=1, max_length=5)
    # start ids and PAD need not be listed
    out = model.generate(x, allowed_token_ids=ok, decoder_start_token_id=999, max_length=5, num_beams=4)
    assert np.isin(out.sequences.cpu().numpy()[:, 1:], ok + [rc.pad_token_id]).all()


# ------------------------------------------------------------------------------------------------ bfloat16
@pytest.fixture(scope="module")
def bf16(dev):
    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    px, *_ = batch(rc, B, 12, seed=21)
    yield rc, p, model, px
    model.release_decode_plans()


@pytest.mark.parametrize("K", [1, 4])
def test_bf16_emits_only_listed_ids(bf16, K):
    """bfloat16 (the granule top-k on the shortlist GEMM's partials for beam 4): every emitted id lies in A or is PAD; shapes and step
    count as in float32.  EOS is suppressed to the end (min_length = max_length), so no hypothesis can finish before the forced EOS and
    the search takes max_length - 1 steps whatever the precision."""
    rc, p, model, px = bf16
    L_ = 10
    kw = dict(max_length=L_, num_beams=K, decoder_start_token_id=999, min_length=L_)
    A, full, ref = _case_A(rc, p, px, kw, seed=19)
    out = model.generate(px.numpy(), allowed_token_ids=A, **kw)
    seq = out.sequences.cpu().numpy()
    assert seq.shape == (B, L_) == _seq(ref, kw).shape and (seq[:, 0] == 999).all()
    assert np.isin(seq[:, 1:], np.concatenate([A, [rc.pad_token_id]])).all(), seq
    print(f"bf16 num_beams={K}: agreement with the fp32 masked oracle {(seq == _seq(ref, kw)).mean():.2f}")
    if K > 1:
        assert tuple(out.scores.shape) == (B,) and bool(torch.isfinite(out.scores).all())
        assert out["steps"] == ref.steps == L_ - 1
        assert (seq[:, -1] == rc.eos_token_id).all()
    plain = model.generate(px.numpy(), **kw).sequences.cpu().numpy()
    assert not np.isin(plain[:, 1:-1], A).all()   # the plain call does leave A: the argument is what confined it


def test_bf16_one_decoder_step_picks_the_candidates_of_the_gathered_full_logits(bf16):
    """One bfloat16 decoder step, head over the shortlist against the full-vocabulary head gathered at A: per row the top-2K id sets
    agree wherever the gap between the 2K-th and the (2K+1)-th gathered value exceeds 4x the measured max difference between the two
    logit arrays (the margin rule of test_generate_bf16_agrees_with_fp32_oracle_on_a_trained_model)."""
    from mic_amd import ops

    rc, p, model, px = bf16
    dev, st = model.device, model.store
    K, L_ = 4, 6
    R, k = B * K, 2 * K
    A = _map(300, 23, st.V)
    sl = model._shortlist(A)
    sl.refresh()
    ehs = model.encode(px.numpy())["last_hidden_state"].to(model.dtype)
    toks = torch.randint(4, st.V, (R,), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    pos = torch.zeros(R, dtype=torch.int32, device=dev)
    res = {}
    for which in ("full", "short"):
        cache = model.init_cache(R, L_)
        model._decode_set_encoder(cache, ehs.reshape(B * st.S, st.d), B, K)
        logits, stat = model._decode_step(cache, toks, pos, stats=True, shortlist=sl if which == "short" else None)
        torch.cuda.synchronize()
        res[which] = (logits.clone(), stat.clone())
    cols = torch.from_numpy(A).long().to(dev)
    gathered = res["full"][0][:R].float()[:, cols]
    short = res["short"][0][:R, : sl.Ns].float()
    err = (gathered - short).abs().max().item()
    print(f"bf16 decoder step: max |shortlist logit - gathered full-vocabulary logit| = {err:.3g} (logit scale {gathered.abs().max().item():.3g})")
    tv, ti = torch.empty((R, k), device=dev), torch.empty((R, k), dtype=torch.int32, device=dev)
    ops.row_topk_tiles(res["short"][0], res["short"][0].stride(0), sl.Ns, res["short"][1], k, tv, ti, R, eos_token_id=sl.column(rc.eos_token_id),
                       token_map=sl.map)
    torch.cuda.synchronize()
    srt = gathered.sort(dim=1, descending=True)
    gap = (srt.values[:, k - 1] - srt.values[:, k]).cpu().numpy()
    decisive = gap > 4 * err
    want = np.sort(A[srt.indices[:, :k].cpu().numpy()], axis=1)
    got = np.sort(ti.cpu().numpy(), axis=1)
    print(f"   {int(decisive.sum())}/{R} rows have a 2K-th / (2K+1)-th gap > 4x that")
    assert np.isin(got, A).all()
    assert np.array_equal(got[decisive], want[decisive])
