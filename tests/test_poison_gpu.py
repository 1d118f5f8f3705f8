"""Scratch poisoning on the device: {entry point} x {mode} x {NaN, loud finite values}.

Buffers outlive calls (`Engine.buf`, the fp8 operand state, decode plans, the Trainer's scratch), and a fresh model holds zeros in all of
them — so every model-level test that builds its own model is blind to a forgotten zeroing or a reduction over a buffer's capacity
instead of its valid rows.  Here every case runs a warm-up so that the buffers exist, poisons every SCRATCH tensor and region of the
inventory (tests/util_poison.py: one contract per tensor, no catch-all), runs the measured call and compares it with the same call on a
twin that has the same call history and was never poisoned — and, where no legitimate state exists (fp32, bf16), with a fresh model.
Deterministic outputs bit for bit, atomically summed gradient leaves within 2e-4 x the leaf's maximum, no new NaN / Inf; every REST
region holds its rest value after every call, also after one a host check refused.

  engine passes    loss_and_grads and loss_only: fp32 padded / compact head, bf16 padded / compact / packed, fp8 delayed and current
                   (packed) with MIC_FP8_HEAD all and 0; label smoothing 0 and 0.1; dropout on, fixed seed
  Trainer          a train_step, an eval_step, a train_step: overlapped and one-launch optimizer, accumulate_steps=2, max_grad_norm,
                   param_groups with a frozen encoder; ParamStore.grad is poisoned whole (every live segment is overwritten)
  inference        __call__ and encode; decode through the cache protocol with the slots behind cache_index of the caller's cache
                   poisoned before every step; generate (greedy, sampling, beam 4, two languages, num_return_sequences=3, a shortlist)
                   with MIC_DECODE_GRAPHS 0 and 1, three calls, plans / caches / cross K/V poisoned between them
  shape history    no poison: full-length captions then one- and two-token captions; a T = 100 batch then the short one on one engine;
                   a generate call that runs to max_length then one that an EOS bias ends at step 2 — against a fresh model
  the suite bites  one zeroing defeated at a time (ops.zero skips the calls into one buffer): logits[Mc:Mcp], hfc[Mc:Mcp], dhf[:M], the
                   decoder step's LayerNorm statistics — the matching case raises

Nothing here can fault: float buffers take any bit pattern, integer buffers only ever receive 1 (valid in every role the inventory
lists) or, the fixed-point LayerNorm sums, (0, 2^40) — a variance that is huge, never negative."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_poison as U  # noqa: E402

pytestmark = pytest.mark.gpu

B_, T_ = U.B_, U.T_
_FRESH = {}  # outputs of fresh models, computed once and shared by the passes (never modified)


def _fresh(key, make):
    if key not in _FRESH:
        _FRESH[key] = make()
    return _FRESH[key]


def _poison(model, how, trainer=None, scenario=""):
    left = U.poison(U.inventory(model, trainer), how, scenario=scenario, sync=U.sync)
    assert all("carries state" in why for why in left.values()), left  # every integer buffer has a stated role
    return left


def _rest(what, model, trainer=None):
    U.sync()
    U.assert_rest(U.inventory(model, trainer), what)


# ================================================================================================ engine passes
@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("mode", list(U.ENGINE_MODES))
def test_engine_passes_ignore_poisoned_scratch(dev, monkeypatch, mode, ls, how):
    md = U.ENGINE_MODES[mode]
    fp8 = "scaling" in md
    if fp8:
        monkeypatch.setenv("MIC_FP8_HEAD", md["head"])
    rc, A = U.engine_model(mode, dev)
    _, B = U.engine_model(mode, dev)
    warm = U.caption_batch(rc, B_, T_, 31, U.NEAR_FULL)  # nearly every row of every buffer has held something
    bt = {True: U.caption_batch(rc, B_, T_, 32), False: U.caption_batch(rc, B_, T_, 33)}
    for m in (A, B):
        for _ in range(2 if fp8 else 1):  # (delayed scaling: the second pass is the one whose producers emit fp8, into buffers of their own)
            for train in (True, False):
                U.engine_pass(m, rc, mode, warm, ls, train)
        _rest(f"{mode} warm-up", m)
    for train in (True, False):
        what = f"{mode} ls={ls} {how} {'loss_and_grads' if train else 'loss_only'}"
        _poison(A, how)
        got, atomic = U.engine_pass(A, rc, mode, bt[train], ls, train)
        want, _ = U.engine_pass(B, rc, mode, bt[train], ls, train)
        _rest(what + " (poisoned)", A)
        _rest(what + " (twin)", B)
        U.compare(got, want, atomic, what + " against the twin")
        if not fp8:  # no legitimate state from call to call: a fresh model computes the same
            def fresh(train=train):
                _, F = U.engine_model(mode, dev)
                return U.engine_pass(F, rc, mode, bt[train], ls, train)[0]
            U.compare(got, _fresh(("engine", mode, ls, train), fresh), atomic, what + " against a fresh model")
    _poison(A, how)
    U.refused_engine_call(A, rc, bt[True])
    _rest(f"{mode} after a refused call", A)


@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("mode", ["fp32-padded", "bf16-compact", "bf16-packed"])
def test_deferred_embedding_rows_ignore_poisoned_scratch(dev, mode, how):
    """Engine.defer_embed (the data-parallel step): the (id, dh0) rows left for the exchange — ids behind the valid packed rows and at
    masked positions are -1 whatever the id list held before — and the table their deterministic scatter builds from them"""
    rc, A = U.engine_model(mode, dev)
    _, B = U.engine_model(mode, dev)
    warm, bt = U.caption_batch(rc, B_, T_, 31, U.NEAR_FULL), U.caption_batch(rc, B_, T_, 32)
    for m in (A, B):
        m.engine.defer_embed = True
        U.engine_pass(m, rc, mode, warm, 0.1, True)
    _poison(A, how)
    got, atomic = U.engine_pass(A, rc, mode, bt, 0.1, True)
    want, _ = U.engine_pass(B, rc, mode, bt, 0.1, True)
    _rest(f"{mode} deferred embedding rows", A)
    assert (got["embed_rows.ids"] == -1).any() and (got["embed_rows.ids"] >= 0).any()
    U.compare(got, want, atomic, f"{mode} {how} deferred embedding rows against the twin")

    def fresh():
        _, F = U.engine_model(mode, dev)
        F.engine.defer_embed = True
        return U.engine_pass(F, rc, mode, bt, 0.1, True)[0]
    U.compare(got, _fresh(("defer", mode), fresh), atomic, f"{mode} {how} deferred embedding rows against a fresh model")


# ================================================================================================ Trainer
TRAINER_MATRIX = [(c, torch.bfloat16) for c in U.TRAINER_CASES] + [("overlap", torch.float32), ("one_launch", torch.float32)]


@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("case,dtype", TRAINER_MATRIX, ids=[f"{c}-{str(d).split('.')[-1]}" for c, d in TRAINER_MATRIX])
def test_trainer_steps_ignore_poisoned_scratch(dev, case, dtype, how):
    rc, A, trA = U.trainer_pair(case, dtype, dev)
    _, B, trB = U.trainer_pair(case, dtype, dev)
    n = trA.accumulate_steps
    bts = [U.batch_dict(U.caption_batch(rc, B_, T_, 41, U.NEAR_FULL))] + [U.batch_dict(U.caption_batch(rc, B_, T_, 42 + i)) for i in range(4)]
    for tr in (trA, trB):
        for j in range(n):
            tr.train_step(bts[j])
        tr.eval_step(bts[1])
    U.sync()
    # the twins took the same steps; their weights still differ by the summation order of the atomically summed gradients the first
    # optimizer step consumed: B continues from A's state
    U.copy_state(U.inventory(A, trA), U.inventory(B, trB))
    U.sync()
    _rest(f"{case} warm-up", A, trA)
    what = f"Trainer {case} {dtype} {how}"
    _poison(A, how, trA)
    got, atomic = U.trainer_outputs(trA, trA.eval_step(bts[2]), False)
    want, _ = U.trainer_outputs(trB, trB.eval_step(bts[2]), False)
    _rest(what + " eval_step", A, trA)
    U.compare(got, want, atomic, what + " eval_step")
    for j in range(n):
        _poison(A, how, trA)  # ParamStore.grad whole: every live segment is overwritten, not accumulated into
        got, atomic = U.trainer_outputs(trA, trA.train_step(bts[3 + j]), True)
        want, _ = U.trainer_outputs(trB, trB.train_step(bts[3 + j]), True)
        _rest(what + f" train_step micro-step {j}", A, trA)
        if j == n - 1:
            U.loosen_weights(got, want, trA, clipped=trA.max_grad_norm is not None)
        U.compare(got, want, atomic, what + f" train_step micro-step {j}")
    assert trA.step == trB.step == 2


# ================================================================================================ inference: __call__, encode, decode
@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_forward_and_encode_ignore_poisoned_scratch(dev, dtype, how):
    from util_small import make_pair

    rc, _, A = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _, _, B = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    w = U.caption_batch(rc, B_, T_, 51, "full")
    px, labels, mask, dec_in = U.caption_batch(rc, B_, T_, 52)

    def forward(m):
        o = m(px.numpy(), decoder_input_ids=dec_in.numpy(), decoder_attention_mask=mask.numpy())
        U.sync()
        return {"logits": o.logits.detach().cpu()}

    def encode(m):
        o = m.encode(px.numpy())
        U.sync()
        return {"last_hidden_state": o.last_hidden_state.detach().cpu(), "pooler_output": o.pooler_output.detach().cpu()}

    for m in (A, B):
        m(w[0].numpy(), decoder_input_ids=w[3].numpy(), decoder_attention_mask=w[2].numpy())
        m.encode(w[0].numpy())
    for name, call in (("__call__", forward), ("encode", encode)):
        what = f"{name} {dtype} {how}"
        _poison(A, how)
        got, want = call(A), call(B)
        _rest(what, A)
        U.compare(got, want, (), what + " against the twin")

        def fresh(call=call):
            return call(make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)[2])
        U.compare(got, _fresh((name, dtype), fresh), (), what + " against a fresh model")


@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_decode_cache_protocol_ignores_poisoned_scratch_and_cache_tail(dev, dtype, how):
    from util_small import make_pair

    rc, _, A = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _, _, B = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    Lmax, steps = 8, 6

    def sequence(m, seed, how=None):
        """`steps` cached decode() calls on a new cache; how: poison the engine's scratch and the cache's tail before every step"""
        px, labels, mask, dec_in = U.caption_batch(rc, B_, T_, seed, "full")
        ehs = m.encode(px.numpy()).last_hidden_state
        cache = m.init_cache(B_, Lmax)
        out = {}
        for t in range(steps):
            if how is not None:
                # (step 0 projects the cross K/V anew; from then on they and the encoder states are the sequence's state)
                _poison(m, how, scenario="" if t == 0 else "decode")
                U.poison_user_cache(cache, how)
                U.sync()
            pos = np.full((B_, 1), t, dtype=np.int32)
            o = m.decode(dec_in[:, t: t + 1].numpy(), (ehs,), decoder_position_ids=pos, past_key_values=cache)
            U.sync()
            assert cache["cache_index"] == t + 1
            out[f"logits{t}"] = o.logits.detach().cpu()
            _rest(f"decode step {t}", m)
        return out

    for m in (A, B):
        sequence(m, 61)  # warm: every buffer of the decoder step exists and holds another sequence's values
    what = f"decode {dtype} {how}"
    got, want = sequence(A, 62, how), sequence(B, 62)
    U.compare(got, want, (), what + " against the twin")
    U.compare(got, _fresh(("decode", dtype), lambda: sequence(make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)[2], 62)), (),
              what + " against a fresh model")


# ================================================================================================ inference: generate
GEN_MATRIX = [(c, torch.bfloat16) for c in U.GENERATE_CASES] + [("greedy", torch.float32), ("beam4", torch.float32)]
GEN_IMAGES = 4


def _gen_kw(case):
    return dict(U.GENERATE_CASES[case])


@pytest.mark.parametrize("how", U.PASSES)
@pytest.mark.parametrize("graphs", ["0", "1"])
@pytest.mark.parametrize("case,dtype", GEN_MATRIX, ids=[f"{c}-{str(d).split('.')[-1]}" for c, d in GEN_MATRIX])
def test_generate_ignores_poisoned_plans_caches_and_scratch(dev, monkeypatch, case, dtype, graphs, how):
    from util_small import make_pair

    monkeypatch.setenv("MIC_DECODE_GRAPHS", graphs)
    rc, _, A = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _, _, B = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    kw = _gen_kw(case)
    what = f"generate {case} {dtype} graphs={graphs} {how}"
    try:
        for call in range(3):  # eager, capture + replay, replay: the third call is the graph-replay path
            px = U.pixels(rc, GEN_IMAGES, 70 + call)
            if call > 0:
                _poison(A, how)
            got, want = U.generate_outputs(A, px, kw), U.generate_outputs(B, px, kw)
            _rest(what + f" call {call}", A)
            U.compare(got, want, (), what + f" call {call} against the twin")
        plans = list(A.__dict__.get("_decode_plans", {}).values())
        if case != "sample":  # (one draw per image keeps no plan)
            assert len(plans) == 1 and plans[0].calls == 3 and (len(plans[0].graphs) > 0) == (graphs == "1"), (len(plans), graphs)

        def fresh():
            F = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)[2]
            try:
                return U.generate_outputs(F, U.pixels(rc, GEN_IMAGES, 72), kw)
            finally:
                F.release_decode_plans()
        U.compare(got, _fresh(("generate", case, dtype), fresh), (), what + " call 2 against a fresh model")
    finally:
        A.release_decode_plans()
        B.release_decode_plans()


# ================================================================================================ shape history, no poison
SHORT = [1, 2, 1, 2, 2, 1]


@pytest.mark.parametrize("mode", ["fp32-padded", "fp32-compact", "bf16-padded", "bf16-compact", "bf16-packed"])
def test_short_captions_after_full_length_ones(dev, mode):
    """the same (B, T), so the same buffers: full-length captions, then one- and two-token captions — as on a fresh model"""
    rc, A = U.engine_model(mode, dev)
    full, short = U.caption_batch(rc, B_, T_, 81, U.NEAR_FULL), U.caption_batch(rc, B_, T_, 82, SHORT)
    for train in (True, False):
        U.engine_pass(A, rc, mode, full, 0.1, train)
    for train in (True, False):
        got, atomic = U.engine_pass(A, rc, mode, short, 0.1, train)
        _rest(f"{mode} short captions", A)
        _, F = U.engine_model(mode, dev)
        want, _ = U.engine_pass(F, rc, mode, short, 0.1, train)
        U.compare(got, want, atomic, f"{mode} short captions after full-length ones, train={train}")


def test_short_batch_after_a_tiled_attention_batch(dev):
    """T = 100 (packed rows, tiled attention cores), then the (B, 16) batch on the same engine — as on a fresh model"""
    mode, over = "bf16-packed", dict(max_position_embeddings=128)
    rc, A = U.engine_model(mode, dev, **over)
    long, short = U.caption_batch(rc, B_, 100, 83), U.caption_batch(rc, B_, T_, 84)
    for train in (True, False):
        U.engine_pass(A, rc, mode, long, 0.0, train, T=100)
    for train in (True, False):
        got, atomic = U.engine_pass(A, rc, mode, short, 0.0, train)
        _rest("short batch after T = 100", A)
        _, F = U.engine_model(mode, dev, **over)
        want, _ = U.engine_pass(F, rc, mode, short, 0.0, train)
        U.compare(got, want, atomic, f"short batch after a T = 100 batch, train={train}")


@pytest.mark.parametrize("graphs", ["0", "1"])
@pytest.mark.parametrize("case", ["greedy", "beam4"])
def test_generate_that_stops_at_step_two_after_one_that_ran_to_max_length(dev, monkeypatch, case, graphs):
    """the same plan: two calls that run to max_length (EOS biased away), then — the final_logits_bias of EOS raised — a call whose
    rows all end at step 2, against a fresh model holding the same weights"""
    from util_small import make_pair

    monkeypatch.setenv("MIC_DECODE_GRAPHS", graphs)
    rc, _, A = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _, _, F = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    kw = dict(_gen_kw(case), forced_bos_token_id=996)
    try:
        U.set_eos_bias(A, rc, -1e4)
        for call in range(2):
            o = U.generate_outputs(A, U.pixels(rc, GEN_IMAGES, 90 + call), kw)
            assert (o["sequences"][:, -2] != rc.eos_token_id).all() and (o["sequences"][:, -2] != rc.pad_token_id).all(), o["sequences"]
        for m in (A, F):
            U.set_eos_bias(m, rc, 1e4)
        px = U.pixels(rc, GEN_IMAGES, 92)
        got, want = U.generate_outputs(A, px, kw), U.generate_outputs(F, px, kw)
        _rest("early stop", A)
        U.compare(got, want, (), f"generate {case} graphs={graphs}: EOS at step 2 after calls that ran to max_length")
        # greedy writes PAD at the EOS step itself (gen:504-507); the beam search returns the last of its K kept hypotheses, which ended
        # one step later: either way nothing but PAD from column 4 on, and the forced BOS in column 1
        assert (got["sequences"][:, 1] == 996).all() and (got["sequences"][:, 4:] == rc.pad_token_id).all(), got["sequences"]
        if case == "greedy":
            assert (got["sequences"][:, 2:] == rc.pad_token_id).all(), got["sequences"]
    finally:
        A.release_decode_plans()
        F.release_decode_plans()


# ================================================================================================ REST of the deterministic scatter
def test_deterministic_scatter_workspace_returns_to_rest(dev):
    """mic_embed_rows_add_det leaves owner = INT_MAX, count = 0, last = -1, multi_count = 0 behind (ids once, twice, many times and
    skipped ones), and reads nothing of the multi list that the call itself did not write"""
    from mic_amd import ops

    rows, d, n = 1024, 128, 300
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, rows, (n,), generator=g, dtype=torch.int32)
    ids[:40] = 7      # many occurrences: the multi list
    ids[40:44] = -1   # skipped
    ids[50] = ids[51] = 9
    dh = torch.randn(n, d, generator=g)
    ids, dh = ids.to(dev), dh.to(dev)
    ws = ops.embed_rows_add_det_workspace(rows, dev)
    entry = U.Entry("trainer.det_ws", ws, U.classify("trainer.det_ws"), {"vocab": rows})
    U.assert_rest([entry], "a new workspace")
    outs = []
    for how in (None,) + U.PASSES:
        if how is not None:
            assert not U.poison([entry], how, sync=U.sync)
        table = torch.zeros(rows, d, device=dev)
        ops.embed_rows_add_det(ids, dh, 0.5, table, n, d, ws)
        U.sync()
        U.assert_rest([entry], f"after a call ({how})")
        outs.append({"table": table.cpu()})
    for o in outs[1:]:
        U.compare(o, outs[0], (), "deterministic scatter over a poisoned multi list")


# ================================================================================================ the inventory has no hole
def test_a_buffer_without_a_contract_fails_the_inventory(dev):
    rc, A = U.engine_model("bf16-compact", dev)
    U.engine_pass(A, rc, "bf16-compact", U.caption_batch(rc, B_, T_, 32), 0.0, True)
    U.inventory(A)
    A.engine.buf("brand.new", 4, 8)
    with pytest.raises(U.PoisonError, match="brand.new"):
        U.inventory(A)


# ================================================================================================ the suite bites
class _SkipZero:
    """ops.zero with one call site defeated: calls whose target lies inside the engine buffer named `name` do nothing"""

    def __init__(self, ops, engine, name):
        self.real, self.engine, self.name, self.skipped = ops.zero, engine, name, 0

    def __call__(self, t):
        for key, b in self.engine._bufs.items():
            if isinstance(key, tuple) and key[0] == self.name and b.data_ptr() <= t.data_ptr() < b.data_ptr() + b.numel() * b.element_size():
                self.skipped += 1
                return t
        return self.real(t)


@pytest.mark.parametrize("site,name", [("logits[Mc:Mcp]", "d.logits"), ("hfc[Mc:Mcp]", "d.hfc"), ("dhf[:M]", "db.dhf")])
def test_a_defeated_zeroing_in_the_engine_is_caught(dev, monkeypatch, site, name):
    from mic_amd import ops

    mode = "bf16-compact"
    rc, A = U.engine_model(mode, dev)
    _, B = U.engine_model(mode, dev)
    warm, bt = U.caption_batch(rc, B_, T_, 31, U.NEAR_FULL), U.caption_batch(rc, B_, T_, 32)
    for m in (A, B):
        U.engine_pass(m, rc, mode, warm, 0.0, True)
    want, atomic = U.engine_pass(B, rc, mode, bt, 0.0, True)
    _poison(A, U.NAN)
    got, _ = U.engine_pass(A, rc, mode, bt, 0.0, True)
    U.compare(got, want, atomic, "defences in place")
    skip = _SkipZero(ops, A.engine, name)
    monkeypatch.setattr(ops, "zero", skip)
    _poison(A, U.NAN)
    got, _ = U.engine_pass(A, rc, mode, bt, 0.0, True)
    monkeypatch.undo()
    assert skip.skipped == 1, (site, skip.skipped)
    with pytest.raises(U.PoisonError):
        U.compare(got, want, atomic, f"{site} not zeroed")


def test_a_defeated_reset_of_the_decoder_step_statistics_is_caught(dev, monkeypatch):
    from mic_amd import ops
    from util_small import make_pair

    monkeypatch.setenv("MIC_DECODE_GRAPHS", "0")
    rc, _, A = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _, _, B = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    kw = _gen_kw("beam4")
    try:
        for m in (A, B):
            U.generate_outputs(m, U.pixels(rc, GEN_IMAGES, 70), kw)
        px = U.pixels(rc, GEN_IMAGES, 71)
        want = U.generate_outputs(B, px, kw)
        skip = _SkipZero(ops, A.engine, "g.lnstats")
        monkeypatch.setattr(ops, "zero", skip)
        _poison(A, U.LOUD)
        got = U.generate_outputs(A, px, kw)
        monkeypatch.undo()
        assert skip.skipped >= 2, skip.skipped  # (one reset per decoder step)
        with pytest.raises(U.PoisonError):
            U.compare(got, want, (), "lnst not zeroed")
    finally:
        A.release_decode_plans()
        B.release_decode_plans()
