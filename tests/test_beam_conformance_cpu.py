"""What the beam-step conformance suite stands on, checked without a GPU: the numpy reference of tests/util_beam_ref.py reproduces
oracle.generation_ref.beam_search when it is fed the per-row top-2K candidates of the same scripted decoders; the cases of
tests/util_beam_cases.py reach every branch the suite is there for (counted, not measured); the cases with a length penalty that
goes through pow are admissible (no decision depends on the last two ulps of a divisor); and every seeded defect of the kernel's
bookkeeping is rejected by at least one case.  The kernel itself: tests/test_beam_conformance_gpu.py."""
import functools
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_beam_cases as BC  # noqa: E402
import util_beam_ref as BR  # noqa: E402
from oracle import generation_ref as G  # noqa: E402

F = np.float32
EOS, PAD, START = BC.EOS, BC.PAD, BC.START


# ------------------------------------------------------------------------------------------------ reference against the oracle
class _Recorder(G.ScriptedStepper):
    """a scripted decoder that keeps the logits of every step"""

    def __init__(self, rows, table):
        super().__init__(rows, table)
        self.logits = []

    def step(self, tokens):
        out = super().step(tokens)
        self.logits.append(out)
        return out


def _table(V, seed, eos_from):
    """logits on a coarse grid (exact ties inside a row and across rows) that depend on the step and on the row's history; from step
    `eos_from` on EOS is among the best of most rows"""
    def table(t, hist):
        rng = np.random.RandomState((seed * 7919 + t * 104729 + int(hist.sum()) * 31 + int(hist[-1])) % (2 ** 31))
        x = rng.randint(0, 8, V) / 2.0
        if t >= eos_from and rng.rand() < 0.8:
            x[EOS] = 4.0 + rng.randint(0, 3) / 2.0
        return x
    return table


def _chain_from_logits(logits, B, K, L, lp, early, procs):
    """the search of oracle.generation_ref.beam_search with step_ref as its body: (sequences, scores, steps)"""
    s = BR.init_state(B, K, L, START, PAD)
    cur_len, steps = 1, 0
    while True:
        assert steps < len(logits), "the reference wants more decoder steps than the oracle took"
        V = logits[steps].shape[1]
        logp = G.log_softmax(logits[steps])                                            # gen:850
        logp = G._apply(procs, s["running_seq"].reshape(B * K, -1), logp, cur_len)     # gen:851-856
        logp = (logp + s["running_scores"].reshape(B * K, 1)).astype(F)                # gen:857
        val, idx = G.top_k(logp, 2 * K)                                                # what mic_row_lse_topk hands over, per row
        div_cur, div_L = BR.divisors(cur_len, L, lp)
        s, flags = BR.step_ref(s, val, idx, K, L, V, cur_len, EOS, div_cur, div_L, early)
        steps += 1
        stop, _ = BR.search_stop(flags, cur_len, L, early)
        cur_len += 1
        if stop:
            break
    any_fin = s["finished"].any(axis=1)                                                # gen:980-990
    seq = np.where(any_fin[:, None, None], s["seq"], s["running_seq"])[:, -1]
    scores = np.where(any_fin[:, None], s["scores"], s["running_scores"])[:, -1]
    return seq, scores, steps


@pytest.mark.parametrize("K", BC.KS)
def test_reference_equals_the_oracle(K):
    """whole searches: sequences, score bits and the number of decoder steps"""
    B, V = 2, 2 * K + 7
    n = 0
    for lp in (0.0, 0.5, 1.0, 2.0):
        for early in (True, False):
            for L, eos_from, forced in ((2, 0, False), (9, 2, False), (9, 4, True), (14, 6, False)):
                procs = G.get_logits_processor(2, L, EOS, 7, EOS) if forced else []
                rec = _Recorder(B * K, _table(V, 100 * K + n, eos_from))
                want = G.beam_search(rec, B, K, START, L, PAD, EOS, lp, early, procs)
                seq, scores, steps = _chain_from_logits(rec.logits, B, K, L, lp, early, procs)
                what = f"K={K} lp={lp} early={early} L={L} forced={forced}"
                assert steps == want.steps, what
                assert np.array_equal(seq, want.sequences), what
                assert np.array_equal(scores.astype(F).view(np.int32), want.scores.astype(F).view(np.int32)), what
                n += 1


def test_divisors_are_the_oracle_s():
    """numpy's fp32 pow (gen:910 in the oracle) against fl32(pow64(cur_len, fl32(lp))) for every length at which the cases use the
    penalty (numpy's fp32 pow is not correctly rounded everywhere: 122 ** 1.25 is an ulp off), and the oracle's div_L for the
    penalties fp32 holds exactly"""
    for lp in BC.LP_EXACT + BC.LP_POW:
        for n in range(1, 163 if lp in BC.LP_EXACT else max(BC.LS) + 1):
            assert BR.divisors(n, n, lp)[0] == F(n) ** F(lp), (n, lp)
            if lp != 1.2:
                assert BR.divisors(1, n, lp)[1] == BR.oracle_div_L(n, lp), (n, lp)
    assert any(BR.divisors(1, n, 1.2)[1] != BR.oracle_div_L(n, 1.2) for n in range(2, 163))   # the difference of reading is real


# ------------------------------------------------------------------------------------------------ the cases
COVERAGE = ("top2k_cut_tie",        # rank 2K-1 against 2K of the top-2K ranking decided by the flat index
            "next_cut_tie",         # the next-beam ranking decided by the candidate index
            "merge_tie_old_new",    # a merge tie between an old finished beam and a new candidate, inside the selection
            "merge_tie_new_new",    # a merge tie among new candidates
            "full",                 # all beams finished & early stopping while the launch goes on
            "late_admit",           # early_stopping=False: new finished candidates enter after all beams finished
            "stop_all_finished", "stop_no_improve", "stop_length",
            "group_stops_alone")    # a search of a grouped launch stops while another continues


@functools.lru_cache(maxsize=None)
def _design():
    """(the branch counts, the reference trajectory of every case), computed once for the tests below"""
    stats = Counter()
    return stats, [BR.run_ref(c, stats=stats) for c in BC.all_cases()]


def test_cases_reach_every_branch():
    stats, _ = _design()
    shapes = set()
    for c in BC.all_cases():
        shapes.add((c["K"], c["L"], c["V"], c["items"], c["G"]))
        assert c["lp"] in BC.LP_EXACT + BC.LP_POW and 2 * c["K"] <= c["V"] and c["items"] % (c["G"] or 1) == 0
        for _, val, _ in c["launches"]:
            fin = val[np.isfinite(val) & (val > -1.0e6)]
            assert (fin * 4 == np.round(fin * 4)).all() and fin.min() >= -40 and fin.max() <= 0, c["name"]
    for name in COVERAGE:
        print(f"[coverage] {name}: {stats[name]}")
    for name in COVERAGE:
        assert stats[name] >= 10, (name, stats[name])
    for K in BC.KS:
        for L in BC.LS:
            for V in BC.VS:
                for items, Gr in BC.LAYOUTS:
                    assert 2 * K > V or (K, L, V, items, Gr) in shapes, (K, L, V, items, Gr)
    used = {(c["lp"], c["early"]) for c in BC.all_cases()}
    assert used == {(lp, e) for lp in BC.LP_EXACT + BC.LP_POW for e in (True, False)}
    assert (32, 162, 250054, 5, None) in shapes   # 65 280 B of LDS
    assert any("forced" in c for c in BC.all_cases())


def test_pow_cases_are_admissible():
    """lp not in {0, 1}: moving div_cur and div_L independently by up to 2 ulp changes no integer output of any launch"""
    n = 0
    for c in BC.all_cases():
        if c["lp"] not in BC.LP_EXACT:
            assert BC.admissible(c), c["name"]
            n += 1
    assert n >= 100
    # and the check can fail: -1e7 / 2 ** 2 against an old finished score one ulp below it
    c = BC.base(1, 8, 61, 1, None, 2.0, False, "inadmissible")
    c["state"] = BC._mid_state(1, 1, 8, 2, [[float(BR.ulps((F(-3.0) + BR.NEG) / F(4.0), -1))]])
    c["launches"] = [(2, *BC._cand(1, [[(-3.0, EOS), (-3.25, 7)]]))]
    BR.plan_launches(c)
    assert not BC.admissible(c)


def test_lp_1_2_oracle_reading_changes_no_flag():
    """lp = 1.2: the oracle raises max_length to the Python double 1.2, the C ABI carries fl32(1.2); div_L differs by an ulp and no
    flag, stop or step count of any case moves"""
    n = 0
    for c in BC.all_cases():
        if c["lp"] == 1.2:
            ours, theirs = BR.run_ref(c), BR.run_ref(c, div_L_of=BR.oracle_div_L)
            for a, b in zip(ours, theirs):
                for (sa, da, ta, _), (sb, db, tb, _) in zip(a, b):
                    assert np.array_equal(sa["flags"], sb["flags"]) and (da, ta) == (db, tb), c["name"]
            n += 1
    assert n >= 10


def _same(a, b):
    return all(da == db and ta == tb and all(np.array_equal(sa[k].view(np.int32), sb[k].view(np.int32)) for k in BR.STATE)
               for pa, pb in zip(a, b) for (sa, da, ta, _), (sb, db, tb, _) in zip(pa, pb))


@pytest.mark.parametrize("defect", BR.DEFECTS)
def test_defect_is_rejected(defect):
    """every seeded mistake changes the outputs of at least one case"""
    hits = [c["name"] for c, want in zip(BC.all_cases(), _design()[1]) if not _same(want, BR.run_ref(c, defect=defect))]
    print(f"[defect] {defect}: rejected by {len(hits)} cases, first: {hits[0] if hits else None}")
    assert hits, defect
