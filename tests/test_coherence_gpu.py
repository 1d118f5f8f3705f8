"""Weight coherence on the device: {way the weights moved} x {derived copy} x {mode}.

The product keeps copies derived from the fp32 master weights and refreshes them lazily or on side streams; a copy that misses one
refresh gives finite, plausible, wrong numbers that no kernel suite and no oracle comparison (they start from freshly loaded weights)
can see.  tests/util_coherence.py holds the inventory — one checker per derived copy, each against the reference the kernel suites
already use, bit for bit or within that reference's bound — and one driver per event:

  derived copies  lp (ParamStore.refresh_lp / the AdamW kernels' p_lp), shared_T (Engine.shared_T / refresh_shared_T on the aux
                  stream), ln_folds (Engine.ln_folded), shortlist (Shortlist.refresh), fp8 (Fp8State.begin_pass / refresh_weights /
                  wait), params (model.params / invalidate_params_cache)
  events          E1 train_step (overlapped optimizer, several buckets), E2 the optimizer as one launch, E3 accumulate_steps=2 (the
                  first micro-step moves nothing), E4 max_grad_norm, E5 param_groups with a frozen encoder, E6 the params setter,
                  E7 restore_checkpoint, E8 a step that raised after some optimizer passes, E9 two events back to back
  modes           fp32, bf16, bf16 with a vocabulary wide enough for the NT head backward (E^T exists), fp8 GEMMs under delayed and
                  current scaling (d 256: the fp8 head is on)

White box (`test_every_derived_copy_follows`): the model is warm — 2 train steps, a beam search and a shortlist beam search called twice
each, so every copy exists and captured decoder steps point into them — then the event, then every checker of the mode.
Black box (`test_warm_model_equals_a_twin_holding_its_weights`): after the event a fresh model that is handed A's parameters must
agree with A bit for bit on encode, teacher-forced decode, the eval_step loss and generate (beam, shortlist beam, greedy, sampling),
A replaying the decode plans and graphs it captured before the weights moved.
The checkers bite (`test_checkers_reject_*`): with the refresh defeated — the version does not advance, or the lp cast is skipped —
the checkers raise.  Stale data only: nothing faults."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_coherence as C  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [f"{m}-{e}" for m, e in C.MATRIX]


@pytest.mark.parametrize("mode,event", C.MATRIX, ids=IDS)
def test_every_derived_copy_follows(dev, monkeypatch, tmp_path, mode, event):
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    ctx = C.prepare(mode, event, dev, tmp_path)
    info = C.DRIVERS[event](ctx)
    C.run_checkers(ctx, info)
    ctx.model.release_decode_plans()


@pytest.mark.parametrize("mode,event", C.MATRIX, ids=IDS)
def test_warm_model_equals_a_twin_holding_its_weights(dev, monkeypatch, tmp_path, mode, event):
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    ctx = C.prepare(mode, event, dev, tmp_path)
    C.DRIVERS[event](ctx)
    C.check_twin(ctx)
    ctx.model.release_decode_plans()


def _raises(checker, ctx):
    with pytest.raises(AssertionError):
        checker(ctx, {})


def test_checkers_reject_copies_whose_version_did_not_advance(dev, monkeypatch, tmp_path):
    """the weights are replaced while `refresh_lp` casts but does not advance `ParamStore.version`: lp is right, E^T, the LayerNorm
    folds and the shortlist are those of the old weights, and their checkers say so"""
    from mic_amd import ops

    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    ctx = C.prepare("bf16wide", "E6_setter", dev, tmp_path)
    st = ctx.model.store
    C.run_checkers(ctx, {}, changed=False)  # all up to date, at the version the warm-up left
    monkeypatch.setattr(st, "refresh_lp", lambda: ops.cast(st.master, st.lp))
    v0 = st.version
    C.ev_setter(ctx)
    assert st.version == v0
    C.check_lp(ctx, {})
    for row in ("shared_T", "ln_folds", "shortlist"):
        _raises(C.CHECKERS[row], ctx)
    monkeypatch.undo()
    ctx.model.invalidate_params_cache()  # the version advances: everything follows
    C.run_checkers(ctx, {}, rows=("lp", "shared_T", "ln_folds", "shortlist"))
    ctx.model.release_decode_plans()


def test_checkers_reject_an_lp_that_missed_its_cast(dev, monkeypatch, tmp_path):
    """the weights are replaced while `refresh_lp` advances the version but skips the cast: lp is the old weights' copy"""
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    ctx = C.prepare("bf16", "E6_setter", dev, tmp_path)
    st = ctx.model.store

    def no_cast():
        st.version += 1
    monkeypatch.setattr(st, "refresh_lp", no_cast)
    C.ev_setter(ctx)
    _raises(C.check_lp, ctx)
    monkeypatch.undo()
    st.refresh_lp()
    C.run_checkers(ctx, {})
    ctx.model.release_decode_plans()
