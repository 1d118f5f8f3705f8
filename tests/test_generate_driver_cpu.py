"""The host pieces of generate()'s decode-chain driver, without a GPU: the step loop (`_run_chain`) against a literal transcription
of the four loops it replaced, the beam epilogue (`_beam_result`) against the four expressions it replaced, on CPU tensors, and the
decode-plan keys (`_plan_key`) against the tuples the strategies used to spell out."""
import types

import pytest
import torch

from mic_amd import generation_clip_vision_utils as GU

Mixin = GU.FlaxCLIPVisionMBartGenerationMixin
_POLL = 8  # the transcriptions below are literal: the poll distance as it was when they were written
NEG = -1.0e7


# ------------------------------------------------------------------------------------------------ the loop
class _Plan:
    """stand-in for a decode plan: writes down what the loop asks of it"""

    def __init__(self, log):
        self.calls, self.log = 3, log

    def run_step(self, cur_len, fn, use_graphs):
        self.log.append(("run_step", cur_len, bool(use_graphs)))
        fn()


def _stop_after(log, last_step):
    """stopped(): written down when consulted; true once step `last_step` has been issued (None: never)"""
    def stopped():
        issued = [e[1] for e in log if e[0] == "step"]
        log.append(("stopped?", issued[-1] if issued else 0))
        return last_step is not None and bool(issued) and issued[-1] >= last_step
    return stopped


def _poll_first(plan, step, max_length, stopped, use_graphs):
    """the loop of `_greedy_search` and `_sample_group` as it was: the poll at the head of the body"""
    cur_len = 1
    while cur_len < max_length:
        if (cur_len - 1) % _POLL == 0 and cur_len > 1 and stopped():
            break
        plan.run_step(cur_len, step(cur_len), use_graphs and cur_len > 1)
        cur_len += 1
    plan.calls += 1


def _poll_last(plan, step, max_length, stopped, use_graphs):
    """the two loops of `_beam_search` as they were: the poll at the foot of the body"""
    cur_len = 1
    while cur_len < max_length:
        plan.run_step(cur_len, step(cur_len), use_graphs and cur_len > 1)
        cur_len += 1
        if cur_len < max_length and (cur_len - 1) % _POLL == 0 and stopped():
            break
    plan.calls += 1


@pytest.mark.parametrize("old_loop", [_poll_first, _poll_last])
@pytest.mark.parametrize("use_graphs", [False, True])
@pytest.mark.parametrize("last_step", [None, 3, 8, 12, 16])  # never / before step 9 / just before it / between 9 and 17 / just before 17
@pytest.mark.parametrize("max_length", [2, 9, 10, 17, 20])
def test_run_chain_equals_the_loops_it_replaced(max_length, last_step, use_graphs, old_loop):
    assert GU._POLL == _POLL
    want, got = [], []
    plan = _Plan(want)
    old_loop(plan, lambda cur_len: (lambda: want.append(("step", cur_len))), max_length, _stop_after(want, last_step), use_graphs)
    assert plan.calls == 4
    plan = _Plan(got)
    GU._run_chain(plan, lambda cur_len: got.append(("step", cur_len)), max_length, _stop_after(got, last_step), use_graphs)
    assert plan.calls == 4
    assert got == want
    # the transcription itself says what the issue says of it
    issued = [e[1] for e in got if e[0] == "step"]
    polls = [e[1] + 1 for e in got if e[0] == "stopped?"]  # the step in front of which the flag was read
    assert all(p in (9, 17) for p in polls) and polls == [p for p in (9, 17) if p < max_length][:len(polls)]
    stop_at = next((p for p in (9, 17) if last_step is not None and last_step < p), None)
    assert issued == list(range(1, min(max_length, stop_at or max_length)))
    assert [e[2] for e in got if e[0] == "run_step"] == [use_graphs and s > 1 for s in issued]


# ------------------------------------------------------------------------------------------------ the beam epilogue
def _n_best_then(out_seq, out_scores, n_best):
    """`_n_best` as it was"""
    return out_seq.flip(1)[:, :n_best].contiguous(), out_scores.flip(1)[:, :n_best].contiguous()


def _old_plain(slices, n_best, max_length):
    """the epilogue of the sliced / unsliced branch of `_beam_search` as it was"""
    outs = []
    for t in slices:
        any_fin = t["finished"].bool().any(dim=1)
        out_seq = torch.where(any_fin[:, None, None], t["seq"], t["running_seq"])
        out_scores = torch.where(any_fin[:, None], t["scores"], t["running_scores"])
        if n_best > 1:
            out_seq, out_scores = _n_best_then(out_seq, out_scores, n_best)
            outs.append((out_seq.reshape(-1, max_length), out_scores.reshape(-1)))
            continue
        outs.append((out_seq[:, -1], out_scores[:, -1]))
    return torch.cat([o[0] for o in outs]).contiguous(), torch.cat([o[1] for o in outs]).contiguous()


def _old_grouped(t, n_best, max_length, n_img, G):
    """the epilogue of the `lang` branch of `_beam_search` as it was"""
    any_fin = t["finished"].bool().any(dim=1)
    if n_best > 1:
        out_seq, out_scores = _n_best_then(torch.where(any_fin[:, None, None], t["seq"], t["running_seq"]),
                                           torch.where(any_fin[:, None], t["scores"], t["running_scores"]), n_best)
        return (out_seq.view(n_img, G, n_best, max_length).transpose(0, 1).reshape(G, n_img * n_best, max_length),
                out_scores.view(n_img, G, n_best).transpose(0, 1).reshape(G, n_img * n_best))
    out_seq = torch.where(any_fin[:, None, None], t["seq"], t["running_seq"])[:, -1]
    out_scores = torch.where(any_fin[:, None], t["scores"], t["running_scores"])[:, -1]
    return out_seq.view(n_img, G, max_length).transpose(0, 1).contiguous(), out_scores.view(n_img, G).transpose(0, 1).contiguous()


def _final_state(items, K, L, seed):
    """a beam search's final state for `items` items: item 0 holds no finished hypothesis, item 1 a single one (the other slots as
    they are initialised: PAD rows, score NEG), item 2 two, every later item K; finished scores sorted ascending (best last)"""
    g = torch.Generator().manual_seed(seed)
    t = {"running_seq": torch.randint(4, 900, (items, K, L), generator=g, dtype=torch.int32),
         "running_scores": -torch.rand(items, K, generator=g).sort(dim=1, descending=True).values,
         "seq": torch.full((items, K, L), 1, dtype=torch.int32), "scores": torch.full((items, K), NEG),
         "finished": torch.zeros((items, K), dtype=torch.int32)}
    for i in range(items):
        n = (0, 1, 2)[i] if i < 3 else K
        if n:
            t["seq"][i, K - n:] = torch.randint(4, 900, (n, L), generator=g, dtype=torch.int32)
            t["scores"][i, K - n:] = -torch.rand(n, generator=g).sort(descending=True).values
            t["finished"][i, K - n:] = 1
    return t


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous() == want.is_contiguous(), (got.shape, want.shape)
    assert torch.equal(got, want)


@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("n_best", [1, 2, 4])
def test_beam_result_of_a_plain_call(n_best, slices):
    K, L = 4, 7
    state = [_final_state(5, K, L, seed=10 * n_best + s) for s in range(slices)]
    want_seq, want_scores = _old_plain(state, n_best, L)
    got = Mixin._beam_result(state, n_best)
    assert set(got) == {"sequences", "scores"} and list(got)[0] == "sequences"
    _same(got["sequences"], want_seq)
    _same(got["scores"], want_scores)
    assert got["sequences"].shape == (5 * slices * n_best, L) and got["sequences"].dtype == torch.int32 and got["scores"].dtype == torch.float32
    # item 0 returns its running hypotheses, item 1 PAD rows with the score NEG past its single finished one
    assert torch.equal(got["sequences"][0], state[0]["running_seq"][0, -1]) and torch.equal(got["sequences"][n_best], state[0]["seq"][1, -1])
    if n_best > 1:
        assert bool((got["sequences"][n_best + 1] == 1).all()) and float(got["scores"][n_best + 1]) == NEG


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n_best", [1, 2, 4])
def test_beam_result_of_a_grouped_call(n_best, G):
    K, L, n_img = 4, 7, 2
    t = _final_state(n_img * G, K, L, seed=100 + 10 * n_best + G)
    want_seq, want_scores = _old_grouped(t, n_best, L, n_img, G)
    got = Mixin._beam_result([t], n_best, G)
    _same(got["sequences"], want_seq)
    _same(got["scores"], want_scores)
    assert got["sequences"].shape == (G, n_img * n_best, L) and got["scores"].shape == (G, n_img * n_best)


# ------------------------------------------------------------------------------------------------ plan keys
def test_plan_keys_are_the_tuples_they_were():
    f32 = torch.float32
    sl = types.SimpleNamespace(key=(301, "0f3c"))
    lang = dict(G=3, start=[2, 2, 2], bos=[996, 995, 994])
    procs = dict(min_length=None, forced_bos=996, forced_eos=2)
    B, K, NS, L, pad, eos, lp, es = 6, 4, 2, 12, 1, 2, 1.0, True
    greedy = (B, L, pad, eos, procs["min_length"], procs["forced_eos"], f32)
    beam = (B, K, NS, L, pad, eos, float(lp), bool(es), procs["min_length"], procs["forced_eos"], f32)
    sample = (2, 3, L, pad, eos, (procs["min_length"], procs["forced_bos"], procs["forced_eos"]), (20, 0.9, 0.7), True, f32)
    for with_lang in (None, lang):
        for with_sl in (None, sl):
            tail = ((("G", 3),) if with_lang else ()) + ((("A",) + sl.key,) if with_sl else ())
            assert Mixin._plan_key("greedy", greedy, with_lang, with_sl) == \
                ("greedy", B, L, pad, eos, procs["min_length"], procs["forced_eos"], f32) + tail
            key = Mixin._plan_key("beam", beam, with_lang, with_sl)
            assert key == ("beam", B, K, NS, L, pad, eos, float(lp), bool(es), procs["min_length"], procs["forced_eos"], f32) + tail
            assert key[3] == NS
    assert Mixin._plan_key("sample", sample) == ("sample", 2, 3, L, pad, eos, (None, 996, 2), (20, 0.9, 0.7), True, f32)
    assert Mixin._plan_key("greedy", greedy, dict(lang, G=1), sl)[-2:] == (("G", 1), ("A", 301, "0f3c"))  # one language is still a grouped call
    # the sampling triple in the key is the one the step applies
    assert Mixin._warp_in_force(dict(top_k=20, top_p=0.9, temperature=0.7), True) == (20, 0.9, 0.7)
    assert Mixin._warp_in_force(dict(top_k=20, top_p=0.9, temperature=0.7), False) == (0, 1.0, 1.0)
    assert Mixin._warp_in_force(dict(top_k=0, top_p=1.0, temperature=None), True) == (0, 1.0, 1.0)


def test_forced_token_of_a_step_counts_in_shortlist_columns():
    sl = types.SimpleNamespace(column=lambda tok: {996: 5, 2: 0}[tok])
    procs = dict(min_length=3, forced_bos=996, forced_eos=2)
    assert Mixin._proc_args(procs, 1, 10) == (996, True) and Mixin._proc_args(procs, 1, 10, sl) == (5, True)
    assert Mixin._proc_args(procs, 9, 10) == (2, False) and Mixin._proc_args(procs, 9, 10, sl) == (0, False)
    assert Mixin._proc_args(procs, 4, 10, sl) == (-1, False)
    assert Mixin._proc_args(procs, 1, 2, sl) == (0, True)  # max_length 2: the forced EOS wins over the forced BOS at step 1
