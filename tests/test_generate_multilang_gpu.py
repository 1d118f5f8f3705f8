"""generate() with a sequence of language ids = that many separate calls on the same images, computed as ONE decode chain
(decoder row = (image * G + g) * num_beams + beam).  Kernel level: mic_row_forced_topk against the scalar forced branch of
mic_row_lse_topk, mic_beam_step_groups against independent mic_beam_step runs.  Model level: float32 against the oracle called
once per language and against separate product calls (bitwise); bfloat16 by group isolation (a language's result does not depend
on its position in the list or on its neighbours)."""
import numpy as np
import pytest
import torch

from test_generate_gpu import _oracle_gen
from util_small import batch, make_pair

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("k", [1, 8, 10, 64])
def test_row_forced_topk_equals_the_scalar_forced_branch(dev, k):
    from mic_amd import ops

    R, V, Vpad = 6, 1003, 1008
    g = torch.Generator().manual_seed(k)
    logits = torch.randn(R, Vpad, generator=g).to(dev)   # read by the scalar kernel's signature only: a forced row scans nothing
    tokens = torch.tensor([0, max(k - 1, 0), k, V - 1, 517, 0], dtype=torch.int32)
    bias = (torch.randn(R, generator=g) * 3).to(dev)
    for rb in (None, bias):
        tv = torch.full((R, k), 7.0, dtype=torch.float32, device=dev)
        ti = torch.full((R, k), -7, dtype=torch.int32, device=dev)
        ops.row_forced_topk(R, k, tokens.to(dev), tv, ti, row_bias=rb)
        for f in sorted(set(tokens.tolist())):
            rv = torch.empty((R, k), dtype=torch.float32, device=dev)
            ri = torch.empty((R, k), dtype=torch.int32, device=dev)
            ops.row_lse_topk(logits, Vpad, V, k, rv, ri, R, forced_token=f, row_bias=rb)
            rows = (tokens == f).nonzero().flatten().to(dev)
            assert torch.equal(tv[rows].view(torch.int32), rv[rows].view(torch.int32)), (k, f)   # bitwise, -inf included
            assert torch.equal(ti[rows], ri[rows]), (k, f)
        assert bool(torch.isinf(tv[:, 1:]).all()) and bool((ti[:, 0].cpu() == tokens).all())


_STATE = ("running_seq", "running_scores", "seq", "scores", "finished", "src_row", "next_token", "flags")
_EOS, _PAD, _NEG = 2, 1, -1.0e7


def _beam_state(items, K, L, dev, groups=None):
    """the state generate() starts a beam search from (gen:751-766), for `items` bookkeeping items"""
    R = items * K
    s = {"running_seq": torch.full((items, K, L), _PAD, dtype=torch.int32), "seq": torch.full((items, K, L), _PAD, dtype=torch.int32),
         "finished": torch.zeros((items, K), dtype=torch.int32), "scores": torch.full((items, K), _NEG),
         "running_scores": torch.tensor([0.0] + [_NEG] * (K - 1)).repeat(items, 1), "next_token": torch.full((R,), 5, dtype=torch.int32),
         "src_row": torch.zeros((R, L), dtype=torch.int32), "flags": torch.zeros((items, 2), dtype=torch.int32),
         "gstate": torch.zeros((groups, 8) if groups else 8, dtype=torch.int32)}
    s["running_seq"][:, :, 0] = 5
    s["src_row"][:, 0] = torch.arange(R, dtype=torch.int32)
    return {k: v.to(dev) for k, v in s.items()}


def _candidates(items, K, V, steps, seed, finish_at):
    """per step ([items*K, 2K] fp32 values, int32 tokens): values from a coarse grid (ties within and across rows), sorted per row,
    distinct tokens per row, an EOS here and there; from step finish_at[item] on every row of that item leads with EOS, so the item
    collects K finished hypotheses there and — with early stopping — stops improving"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(1, steps + 1):
        val = (-t - torch.randint(0, 6, (items * K, 2 * K), generator=g).float() / 4).sort(dim=1, descending=True).values
        idx = torch.stack([torch.randperm(V - 4, generator=g)[: 2 * K] + 4 for _ in range(items * K)]).to(torch.int32)
        rare = torch.rand(items * K, generator=g) < 0.05
        slot = torch.randint(0, 2 * K, (items * K,), generator=g)
        idx[rare.nonzero().flatten(), slot[rare]] = _EOS
        for i in range(items):
            if t >= finish_at[i]:
                rows = slice(i * K, (i + 1) * K)
                idx[rows][idx[rows] == _EOS] = 3   # (3 is never drawn above: tokens stay distinct within a row)
                idx[rows, 0] = _EOS
                val[rows, 0] = val[rows, 0] + 2.0   # above every other candidate of the item
        out.append((val.contiguous(), idx.contiguous()))
    return out


def _step(ops, s, items, K, L, V, cur_len, val, idx, groups=None):
    args = (items, K, L, V, cur_len, _EOS, _PAD, 1.0, True, val, idx, s["running_seq"], s["running_scores"], s["seq"], s["scores"],
            s["finished"], s["src_row"], s["next_token"], s["flags"])
    ops.beam_step(*args, gstate=s["gstate"], groups=groups)   # groups=None: mic_beam_step; an int: mic_beam_step_groups


@pytest.mark.parametrize("K", [4, 12])
def test_beam_step_groups_of_one_is_beam_step(dev, K):
    from mic_amd import ops

    B, L, V, steps = 4, 14, 61, 12
    cands = _candidates(B, K, V, steps, seed=K, finish_at=[8, 7, 8, 6])
    a, b = _beam_state(B, K, L, dev), _beam_state(B, K, L, dev, groups=1)
    for t, (val, idx) in enumerate(cands, start=1):
        val, idx = val.to(dev), idx.to(dev)
        _step(ops, a, B, K, L, V, t, val, idx)
        _step(ops, b, B, K, L, V, t, val, idx, groups=1)
        for name in _STATE:
            assert torch.equal(a[name], b[name]), (name, t)
        assert torch.equal(a["gstate"], b["gstate"][0]), t
    assert int(a["gstate"][3]) == 1 and 1 < int(a["gstate"][4]) < steps   # it stopped on its own, later launches were no-ops
    assert bool(a["finished"].any())


def test_beam_step_groups_equal_independent_searches(dev):
    """three searches interleaved item by item (item = image * 3 + g) against three separate mic_beam_step runs on the de-interleaved
    candidates: equal after every step, also after a search has stopped while the others keep going"""
    from mic_amd import ops

    G, Bi, K, L, V, steps = 3, 3, 3, 14, 61, 12
    items = Bi * G
    stop_at = {0: 9, 1: 4, 2: 6}   # search g: all of its items collect K finished hypotheses at this step
    cands = _candidates(items, K, V, steps, seed=3, finish_at=[stop_at[i % G] for i in range(items)])
    grouped = _beam_state(items, K, L, dev, groups=G)
    single = [_beam_state(Bi, K, L, dev) for _ in range(G)]

    def of_group(x, g, per_row):
        """rows / items of search g out of an item-major tensor"""
        n = K if per_row else 1
        return x.reshape(Bi, G, n, *x.shape[1:])[:, g].reshape(Bi * n, *x.shape[1:])

    def local_rows(src):   # a grouped row id (item * K + beam) as the separate run numbers it ((item // G) * K + beam)
        return (src // K // G) * K + src % K

    for t, (val, idx) in enumerate(cands, start=1):
        _step(ops, grouped, items, K, L, V, t, val.to(dev), idx.to(dev), groups=G)
        for g in range(G):
            s = single[g]
            _step(ops, s, Bi, K, L, V, t, of_group(val, g, True).contiguous().to(dev), of_group(idx, g, True).contiguous().to(dev))
            for name in _STATE:
                got = grouped[name]
                if name in ("src_row", "next_token"):
                    got = of_group(got, g, True)
                else:
                    got = of_group(got.reshape(items, -1), g, False).reshape(s[name].shape)
                if name == "src_row":
                    got = local_rows(got)
                assert torch.equal(got, s[name]), (name, g, t)
            assert torch.equal(grouped["gstate"][g, 3:5], s["gstate"][3:5]), (g, t)
    took = [int(s["gstate"][4]) for s in single]
    assert took == [stop_at[g] for g in range(G)], took   # three different steps, each before the last one
    assert grouped["gstate"][:, 3].tolist() == [1, 1, 1] and grouped["gstate"][:, 4].tolist() == took


# ------------------------------------------------------------------------------------------------ model level, float32
_IMG = dict(B=3, seed=61)


@pytest.fixture(scope="module")
def fp32(dev):
    """(oracle config, oracle params, product model, images): EOS pushed up a little so that searches end at different steps"""
    from mic_amd.params import unflatten_tree

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    p = dict(p)
    flb = p["final_logits_bias"].clone()
    flb[0, rc.eos_token_id] = 0.5
    p["final_logits_bias"] = flb
    model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
    px, *_ = batch(rc, _IMG["B"], 12, seed=_IMG["seed"])
    yield rc, p, model, px
    model.release_decode_plans()


_ORACLE = {}


def _oracle(rc, p, px, tag, **kw):
    """the oracle's result of one (single-language) call, computed once per distinct call"""
    key = (tag,) + tuple(sorted(kw.items()))
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_gen(rc, p, px, px.shape[0], **kw)
    return _ORACLE[key]


def _per_language(kw):
    """the G single-language argument sets of a grouped call"""
    G = max(len(v) for v in kw.values() if isinstance(v, (list, tuple)))
    return [{k: (v[g] if isinstance(v, (list, tuple)) else v) for k, v in kw.items()} for g in range(G)]


def _check_against_oracle(rc, p, model, px, tag, **kw):
    out = model.generate(px.numpy(), **kw)
    calls = _per_language(kw)
    G, B, L = len(calls), px.shape[0], kw["max_length"]
    seq = out.sequences.cpu().numpy()
    assert seq.shape == (G, B, L)
    beam = kw.get("num_beams", 1) > 1
    if beam:
        assert tuple(out.scores.shape) == (G, B) and isinstance(out["steps"], list) and len(out["steps"]) == G
    for g, one in enumerate(calls):
        ref = _oracle(rc, p, px, tag, **one)
        assert np.array_equal(seq[g], ref.sequences if beam else ref), (g, one)
        if beam:
            assert out["steps"][g] == ref.steps, (g, out["steps"], ref.steps)
            assert np.allclose(out.scores[g].cpu().numpy(), ref.scores, rtol=1e-4, atol=1e-4), g
    return out


def test_staggered_stops_equal_the_oracle_and_separate_calls(fp32):
    """four languages whose separate searches stop after 10, 19, 5 and 14 steps: on both sides of the 8- and 16-step polls of the
    stop flags, one running to the end.  Against the oracle per language, and bitwise against four separate product calls (the
    fp32 GEMM's per-element summation order does not depend on the row count, every other decode kernel works per row)."""
    rc, p, model, px = fp32
    ids = [996, 995, 994, 993]
    kw = dict(num_beams=4, max_length=20)
    out = _check_against_oracle(rc, p, model, px, "img", forced_bos_token_id=ids, **kw)
    print("steps per language:", out["steps"])
    assert out["steps"] == [10, 19, 5, 14]
    for g, bos in enumerate(ids):
        one = model.generate(px.numpy(), forced_bos_token_id=bos, **kw)
        assert one["steps"] == out["steps"][g]
        assert torch.equal(one.sequences, out.sequences[g]), g
        assert torch.equal(one.scores, out.scores[g]), (g, (one.scores - out.scores[g]).abs().max().item())


@pytest.mark.parametrize("kw", [dict(decoder_start_token_id=[999, 998], max_length=10),
                                dict(decoder_start_token_id=[999, 998], forced_bos_token_id=[996, 995], max_length=10),
                                dict(decoder_start_token_id=997, forced_bos_token_id=(996, 995, 994), max_length=10),
                                dict(forced_bos_token_id=[996, 995], num_beams=12, max_length=8),   # the streaming top-k's 32-wide build
                                dict(forced_bos_token_id=[996, 995], max_length=2),                 # ForcedEOS wins over the per-row BOS
                                dict(forced_bos_token_id=[996], max_length=10), dict(decoder_start_token_id=(998,), max_length=10)])
def test_language_arguments_against_the_oracle(fp32, kw):
    rc, p, model, px = fp32
    kw = dict(kw)
    kw.setdefault("num_beams", 4)
    out = _check_against_oracle(rc, p, model, px, "img", **kw)
    if kw["max_length"] == 2:
        assert bool((out.sequences[:, :, 1] == rc.eos_token_id).all())


def test_numpy_and_torch_id_arrays_select_the_grouped_call(fp32):
    rc, p, model, px = fp32
    a = model.generate(px.numpy(), forced_bos_token_id=[996, 995], num_beams=4, max_length=10)
    for ids in (np.array([996, 995]), torch.tensor([996, 995], dtype=torch.int32)):
        b = model.generate(px.numpy(), forced_bos_token_id=ids, num_beams=4, max_length=10)
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) and a["steps"] == b["steps"]


def test_greedy_languages_against_the_oracle(fp32):
    rc, p, model, px = fp32
    _check_against_oracle(rc, p, model, px, "img", forced_bos_token_id=[996, 995, 994], num_beams=1, max_length=12)
    _check_against_oracle(rc, p, model, px, "img", decoder_start_token_id=[999, 998], num_beams=1, max_length=12)


def test_generate_languages_helper(fp32):
    from mic_amd.evaluation import generate_languages

    rc, p, model, px = fp32
    langs = {"en_XX": 996, "fr_XX": 995, "de_DE": 994}
    for via, arg in (("forced_bos", "forced_bos_token_id"), ("decoder_start", "decoder_start_token_id")):
        got = generate_languages(model, px.numpy(), langs, via=via, max_length=10, num_beams=4)
        assert list(got) == list(langs)
        for lang, tok in langs.items():
            ref = _oracle(rc, p, px, "img", num_beams=4, max_length=10, **{arg: tok})
            assert np.array_equal(got[lang], ref.sequences), (via, lang)


def test_grouped_plan_graph_replay(fp32, monkeypatch):
    """MIC_DECODE_GRAPHS=1: call 1 of the plan is eager, call 2 captures steps >= 2 and replays them, call 3 only replays — with
    other images and the language list permuted (the ids live in plan tensors refilled per call, step 1 is never captured)"""
    rc, p, model, _ = fp32
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    model.release_decode_plans()
    kw = dict(num_beams=4, max_length=12)
    for call, (seed, ids) in enumerate([(71, [996, 995, 994]), (72, [994, 996, 995]), (73, [995, 994, 996])]):
        px, *_ = batch(rc, _IMG["B"], 12, seed=seed)
        out = _check_against_oracle(rc, p, model, px, seed, forced_bos_token_id=ids, **kw)
        assert len(model._decode_plans) == 1
        plan = next(iter(model._decode_plans.values()))
        assert plan.calls == call + 1
        if call >= 1:
            assert len(plan.graphs) > 0 and 1 not in plan.graphs
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "0")
    eager = model.generate(px.numpy(), forced_bos_token_id=ids, **kw)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.scores, out.scores) and eager["steps"] == out["steps"]
    model.release_decode_plans()


def test_sampling_with_a_language_sequence_is_refused(fp32):
    rc, p, model, px = fp32
    with pytest.raises(NotImplementedError, match="sequence of language ids"):
        model.generate(px.numpy(), do_sample=True, num_beams=1, max_length=6, forced_bos_token_id=[996, 995])
    with pytest.raises(ValueError):
        model.generate(px.numpy(), num_beams=4, max_length=6, forced_bos_token_id=[996, rc.vocab_size])


def test_scalar_calls_around_a_grouped_call_are_unchanged(fp32):
    rc, p, model, px = fp32
    B = px.shape[0]
    kw = dict(num_beams=4, max_length=10, forced_bos_token_id=996)
    ref = _oracle(rc, p, px, "img", **kw)
    ref_greedy = _oracle(rc, p, px, "img", num_beams=1, max_length=12, forced_bos_token_id=995)
    before = model.generate(px.numpy(), **kw)
    model.generate(px.numpy(), num_beams=4, max_length=10, forced_bos_token_id=[995, 996])
    model.generate(px.numpy(), num_beams=1, max_length=12, forced_bos_token_id=[995, 996])
    after = model.generate(px.numpy(), **kw)
    for out in (before, after):
        assert tuple(out.sequences.shape) == (B, 10) and tuple(out.scores.shape) == (B,) and isinstance(out["steps"], int)
        assert np.array_equal(out.sequences.cpu().numpy(), ref.sequences) and out["steps"] == ref.steps
        assert np.allclose(out.scores.cpu().numpy(), ref.scores, rtol=1e-4, atol=1e-4)
    assert torch.equal(before.sequences, after.sequences) and torch.equal(before.scores, after.scores)
    greedy = model.generate(px.numpy(), num_beams=1, max_length=12, forced_bos_token_id=995)
    assert tuple(greedy.sequences.shape) == (B, 12) and np.array_equal(greedy.sequences.cpu().numpy(), ref_greedy)


# ------------------------------------------------------------------------------------------------ model level, bfloat16
@pytest.mark.parametrize("K", [4, 12])   # 4: top-2K from the head GEMM's partials (row_topk_tiles); 12: the streaming top-k
def test_bf16_groups_are_isolated(dev, K):
    """bfloat16: separate calls run their GEMMs at another row count (another K split, other low bits) and a random model's logits tie
    massively, so equality with separate calls is not the criterion.  Group isolation is: a language's sequences, scores and step
    count do not depend on its position in the list or on its neighbours."""
    from mic_amd.params import unflatten_tree

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    p = dict(p)
    flb = p["final_logits_bias"].clone()
    flb[0, rc.eos_token_id] = 0.5
    p["final_logits_bias"] = flb
    model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
    px, *_ = batch(rc, _IMG["B"], 12, seed=_IMG["seed"])
    kw = dict(num_beams=K, max_length=14)
    a_ids, b_ids = [996, 995, 994], [994, 996, 995]
    a = model.generate(px.numpy(), forced_bos_token_id=a_ids, **kw)
    b = model.generate(px.numpy(), forced_bos_token_id=b_ids, **kw)
    for tok in a_ids:
        i, j = a_ids.index(tok), b_ids.index(tok)
        assert torch.equal(a.sequences[i], b.sequences[j]), tok
        assert torch.equal(a.scores[i], b.scores[j]) and a["steps"][i] == b["steps"][j], tok
        assert bool((a.sequences[i][:, 1] == tok).all())
    twice = model.generate(px.numpy(), forced_bos_token_id=[996, 996], **kw)
    assert torch.equal(twice.sequences[0], twice.sequences[1]) and torch.equal(twice.scores[0], twice.scores[1])
    assert twice["steps"][0] == twice["steps"][1] and bool((twice.sequences[:, :, 1] == 996).all())
    model.release_decode_plans()
