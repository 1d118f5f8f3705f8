"""The check on the checker of the decode selection conformance suite; runs without a GPU.
  - fp32 numpy emulations of the kernels' arithmetic (util_decode_ref.emu_*) give the reference's index sequence and lie within the
    derived bounds on every case of util_decode_cases.py (the printed ratios are the emulation's column of
    profiles/decode_conformance_worst_ratio.txt);
  - every case is admissible — the fp64 order is the truth for an fp32 kernel — with zero exceptions;
  - seeded defects, applied to the emulations, are each rejected on a named case, and it is printed which of them the assertions of
    tests/test_ops_gpu.py / tests/test_generate_gpu.py (random normal logits, atol = 2e-5 max) would have accepted;
  - every decode instantiation of the build's resource table in scope is claimed by a case and launched by the GPU module (its
    committed kernel listing).
Out of scope (as in the GPU module): mic_beam_step / mic_beam_step_groups — see tests/test_beam_conformance_cpu.py."""
import fnmatch
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_decode_cases as DC  # noqa: E402
import util_decode_ref as DR  # noqa: E402
import util_rowop_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE_PROFILE = "profiles/decode_conformance_kernel_stats.txt"
F = np.float32


def report(quantity, case, worst, n):
    print(f"[conformance] {quantity}: {case}: worst err/bound {worst:.3g} over {n} elements")


# ------------------------------------------------------------------------------------------------ mic_row_lse_topk
@functools.lru_cache(maxsize=None)
def _lse_rows(V, rows, mode):
    x0, bias = DC.lse_grid_rows(V) if rows == "grid" else DC.lse_edge_rows(V)
    x, sup, eos, raw = DC.lse_mode(x0, mode)
    refs = [DR.proc_ref(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw) for r in range(x.shape[0])]
    emus = [DR.emu_lse_values(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw) for r in range(x.shape[0])]
    return x, bias, sup, eos, raw, refs, emus


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.LSE_V)
def test_row_lse_topk_emulation_and_admissibility(V, dtype):
    for rows in ("grid", "edge"):
        for mode in DC.LSE_MODES:
            x, bias, sup, eos, raw, refs, emus = _lse_rows(V, rows, mode)
            names = DC.BIASES if rows == "grid" else DC.LSE_EDGE_ROWS
            for r, ref in enumerate(refs):
                worst = 0.0
                for k in DC.lse_ks(V):
                    what = f"V={V} {mode} {names[r]} k={k}"
                    assert DR.admissible_topk(ref, k, raw) == [], what
                    val, idx = DR.emu_row_lse_topk(x[r], k, values=emus[r], suppress_eos=sup, eos=eos, raw=raw)
                    w = DR.check_topk(val, idx, ref, k, V, what, "value", log=False)
                    worst = max(worst, w or 0.0)
                if not ref["exact"]:
                    report(f"row_lse_topk/{dtype} value", f"V={V} {mode} {names[r]}", worst, sum(DC.lse_ks(V)))


def test_forced_entries():
    """the forced branch restated (entry 0 = the forced token at 0 + bias, then the lowest indices that skip it at -inf) equals
    ForcedBOS followed by top-k, for the per-row ids and k of the GPU test"""
    for k in DC.FORCED_K:
        for f in DC.FORCED_ROWS.tolist():
            idx = [f] + [t - 1 + (t - 1 >= f) for t in range(1, k)]
            rv, ri = DR.forced_ref(max(k, f) + 2, f, k, -3.5)
            assert ri.tolist() == idx and rv[0] == -3.5 and np.isneginf(rv[1:]).all()


# ------------------------------------------------------------------------------------------------ mic_row_topk_tiles
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("k", DC.TILES_K)
def test_row_topk_tiles_emulation_and_admissibility(k, dtype):
    for nt in DC.tiles_ntiles(k):
        x, bias, eos = DC.tiles_rows(nt, k)
        V = x.shape[1]
        part = RR.tile_partials(x)
        assert part.shape[1] == nt
        for sup, raw in ((False, False), (True, False), (False, True)):
            for r in range(x.shape[0]):
                what = f"ntiles={nt} k={k} row {r}{' suppress_eos' if sup else ''}{' raw' if raw else ''}"
                ref = DR.proc_ref(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw, part=part[r])
                full = DR.proc_ref(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw)
                assert DR.admissible_topk(ref, k, raw) == [] and DR.admissible_topk(full, k, raw) == [], what
                if not (raw and k == 1 and abs(bias[r]) >= DR.BIG_BIAS):  # (there mic_row_lse_topk is the argmax of the logits themselves)
                    assert np.array_equal(DR.topk_ref(ref, k)[1], DR.topk_ref(full, k)[1]), what + ": partials and streaming references disagree"
                val, idx = DR.emu_row_topk_tiles(x[r], part[r], k, bias[r], suppress_eos=sup, eos=eos, raw=raw)
                w = DR.check_topk(val, idx, ref, k, V, what, "value", log=False)
                if w is not None:
                    report(f"row_topk_tiles/{dtype} value", what, w, k)


# ------------------------------------------------------------------------------------------------ mic_warp_thresholds
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.WARP_V)
def test_warp_thresholds_emulation_and_admissibility(V, dtype):
    x = DC.warp_rows(V, dtype)
    for (k, p, T, sup) in DC.warp_combos(V):
        for r in range(x.shape[0]):
            what = f"V={V} {DC.WARP_ROWS[r]} top_k={k} top_p={p} T={T} suppress={sup}"
            y = DR.scaled(x[r], T, sup, 2)
            ref = DR.warp_ref(y, k, p)
            assert ref["margin"] is None or ref["margin"] > ref["delta"], f"{what}: margin {ref['margin']:.3g} delta {ref['delta']:.3g}"
            thr, lim = DR.emu_warp(x[r], T, k, p, suppress_eos=sup, eos=2)
            assert np.array_equal(DR.mask_of(y, thr, lim), ref["keep"]), what
            if k > 0:
                assert ref["n_topk"] == min(k, int(np.isfinite(y).sum())), what


def test_signed_zero_row_keeps_three():
    """the worked example: [+0, -0, -0, +0, -1] with top_k = 3.  The keys without the canonicalisation put the zeros in two bins: thr =
    -0, n_keep = 1, the walk over == counts all four zeros and one token survives; with it the warper's three do"""
    y = DR.scaled(DC.ZERO_ROW, 1.0)
    keep = DR.warp_ref(y, 3, 1.0)["keep"]
    assert keep.tolist() == [True, True, True, False, False]
    assert DR.mask_of(y, *DR.emu_warp(DC.ZERO_ROW, 1.0, 3, 1.0, defect="no_canon")).sum() == 1
    assert np.array_equal(DR.mask_of(y, *DR.emu_warp(DC.ZERO_ROW, 1.0, 3, 1.0)), keep)


# ------------------------------------------------------------------------------------------------ mic_sample_rows
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.SAMPLE_V)
@pytest.mark.parametrize("R", DC.SAMPLE_R)
def test_sample_rows_emulation_and_admissibility(R, V, dtype):
    from oracle import generation_ref as G

    x = DC.sample_rows_of(R, V)
    key = G.prng_split(G.prng_key(DC.SAMPLE_KEY_SEED.get((R, V), R + V)))[0]
    assert np.array_equal(DR.kernel_bits(key, R * V), G.random_bits(key, R * V))
    for variant in DC.SAMPLE_VARIANTS:
        s = DR.sample_setup(x, variant)
        ref, ok, info = DR.sample_ref(x, key, **s)
        assert all(ok), f"R={R} V={V} {variant}: gap / bound per row {info}"
        assert np.array_equal(DR.emu_sample(x, key, **s), ref), f"R={R} V={V} {variant}"
        if variant == "topk1_topk3":
            kept = [DR.mask_of(DR.scaled(x[r], 1.0), s["thr"][r], s["lim"][r]).sum() for r in range(R)]
            assert kept[0] == 1 and kept[1] == min(3, V), kept


# ------------------------------------------------------------------------------------------------ seeded defects
def _old_topk_accepts(defect, **kw):
    """tests/test_ops_gpu.py test_row_lse_topk: random normal fp32 logits at V = 1003, k = 8, indices equal and values within
    2e-5 max |ref| of an fp32 numpy reference"""
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(1003) * 3).astype(F).astype(np.float64)
    val, idx = DR.emu_row_lse_topk(x, 8, kw.get("bias", 0.0), suppress_eos=kw.get("sup", False), eos=2, defect=defect)
    r = DR.proc_ref(x, kw.get("bias", 0.0), suppress_eos=kw.get("sup", False), eos=2)
    rv, ri, _ = DR.topk_ref(r, 8)
    return bool(np.array_equal(idx, ri) and np.abs(val - rv).max() <= 2e-5 * np.abs(rv).max())


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_defects_of_the_streaming_top_k_are_rejected():
    accepted = {}
    # tie broken by highest index: the 40 equal maxima
    x, bias = DC.lse_edge_rows(2049)
    ref = DR.proc_ref(x[0], bias[0])
    _rejected(lambda: DR.check_topk(*DR.emu_row_lse_topk(x[0], 8, bias[0], defect="highest_index"), ref, 8, 2049, "highest_index", "value", log=False))
    accepted["tie broken by highest index"] = _old_topk_accepts("highest_index")
    # EOS not suppressed: EOS is the row maximum
    xg, bg = DC.lse_grid_rows(2049)
    xm, sup, eos, _ = DC.lse_mode(xg, "eos_max")
    ref = DR.proc_ref(xm[0], bg[0], suppress_eos=True, eos=eos)
    _rejected(lambda: DR.check_topk(*DR.emu_row_lse_topk(xm[0], 8, bg[0], suppress_eos=True, eos=eos, defect="no_eos"), ref, 8, 2049, "no_eos", "value", log=False))
    accepted["EOS not suppressed"] = _old_topk_accepts("no_eos", sup=True)   # column 2 of a random row is rarely in the top 8
    # bias added before the log-softmax: the rows with a running score
    for r in (2, 3):
        ref = DR.proc_ref(xg[r], bg[r])
        _rejected(lambda: DR.check_topk(*DR.emu_row_lse_topk(xg[r], 8, bg[r], defect="bias_first"), ref, 8, 2049, "bias_first", "value", log=False))
    accepted["bias added before the log-softmax"] = _old_topk_accepts("bias_first", bias=-3.5)
    # lse missing the tail chunk: V = 2049 has one column in it; the all-equal row gives it 1 / V of the mass
    ref = DR.proc_ref(x[1], bias[1])
    _rejected(lambda: DR.check_topk(*DR.emu_row_lse_topk(x[1], 8, bias[1], defect="no_tail"), ref, 8, 2049, "no_tail", "value", log=False))
    accepted["lse missing the tail chunk"] = _old_topk_accepts("no_tail")
    for k, v in accepted.items():
        print(f"[old tolerance] {k}: {'ACCEPTED' if v else 'rejected'} by the assertion of tests/test_ops_gpu.py::test_row_lse_topk")
    assert accepted["tie broken by highest index"], "random normal fp32 logits have no ties: the old test cannot see the tie rule"


def test_tau_from_the_kth_granule_is_rejected_under_suppress_eos():
    for k in (8, 16):
        x, bias, eos = DC.tiles_rows(k + 1, k)
        part = RR.tile_partials(x)
        ref = DR.proc_ref(x[4], bias[4], suppress_eos=True, eos=eos, part=part[4])
        good = DR.emu_row_topk_tiles(x[4], part[4], k, bias[4], suppress_eos=True, eos=eos)
        DR.check_topk(*good, ref, k, x.shape[1], "eos_tau", "value", log=False)
        bad = DR.emu_row_topk_tiles(x[4], part[4], k, bias[4], suppress_eos=True, eos=eos, defect="tau_k")
        _rejected(lambda: DR.check_topk(*bad, ref, k, x.shape[1], "eos_tau", "value", log=False))
    # the old test (random normal logits, EOS = column 2): the defect is invisible unless column 2 is a top granule's maximum
    rng = np.random.default_rng(1)
    xo = (rng.standard_normal((1, 1003)) * 3).astype(F).astype(np.float64)
    po = RR.tile_partials(xo)
    ro = DR.proc_ref(xo[0], 0.0, suppress_eos=True, eos=2, part=po[0])
    vb, ib = DR.emu_row_topk_tiles(xo[0], po[0], 8, 0.0, suppress_eos=True, eos=2, defect="tau_k")
    ok = np.array_equal(ib, DR.topk_ref(ro, 8)[1])
    print(f"[old tolerance] tau from the k-th granule: {'ACCEPTED' if ok else 'rejected'} by tests/test_ops_gpu.py::test_head_rowstat_topk_and_ce_from_tile_partials")


def test_defects_of_the_warpers_are_rejected():
    x = DC.warp_rows(1025, "f32")
    # radix keys without the zero canonicalisation: the signed-zero row, top-k and top-p
    for k, p in ((3, 1.0), (0, 0.5)):
        y = DR.scaled(x[1], 1.0)
        keep = DR.warp_ref(y, k, p)["keep"]
        assert np.array_equal(DR.mask_of(y, *DR.emu_warp(x[1], 1.0, k, p)), keep)
        assert not np.array_equal(DR.mask_of(y, *DR.emu_warp(x[1], 1.0, k, p, defect="no_canon")), keep), (k, p)
    # n_keep off by one: the ties row, the cut inside the entries equal to the threshold
    y = DR.scaled(x[3], 1.0)
    keep = DR.warp_ref(y, 100, 1.0)["keep"]
    assert np.array_equal(DR.mask_of(y, *DR.emu_warp(x[3], 1.0, 100, 1.0)), keep)
    assert not np.array_equal(DR.mask_of(y, *DR.emu_warp(x[3], 1.0, 100, 1.0, defect="n_keep_off")), keep)
    # the old test: random normal logits; |kept - reference| <= 1
    rng = np.random.default_rng(2)
    xo = (rng.standard_normal(1003) * 2).astype(F).astype(np.float64)
    yo = DR.scaled(xo, 1.0)
    for d in ("no_canon", "n_keep_off"):
        diff = abs(int(DR.mask_of(yo, *DR.emu_warp(xo, 1.0, 50, 1.0, defect=d)).sum()) - 50)
        print(f"[old tolerance] warpers {d}: {'ACCEPTED' if diff <= 1 else 'rejected'} by tests/test_generate_gpu.py::test_warp_thresholds_match_oracle_warpers (diff {diff})")
        assert diff <= 1


def test_swapped_counter_halves_are_rejected_at_odd_sizes():
    from oracle import generation_ref as G

    R, V = 3, 1023
    x = DC.sample_rows_of(R, V)
    key = G.prng_split(G.prng_key(R + V))[0]
    ref, ok, _ = DR.sample_ref(x, key)
    assert all(ok) and np.array_equal(DR.emu_sample(x, key), ref)
    assert not np.array_equal(DR.emu_sample(x, key, defect="halves_swapped"), ref)
    x4 = DC.sample_rows_of(4, V)
    assert np.array_equal(DR.emu_sample(x4, key, defect="halves_swapped"), DR.emu_sample(x4, key)), "an even R * V is not affected"
    print("[old tolerance] threefry halves swapped: rejected by tests/test_generate_gpu.py::test_sample_rows_matches_jax_threefry_oracle (it has R * V = 3009)")


# ------------------------------------------------------------------------------------------------ coverage
def test_cases_meet_the_issue_floor():
    assert set(DC.LSE_V) == {7, 8, 9, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16389} and set(DC.LSE_K) == {1, 2, 8, 9, 16, 17, 32, 33, 64}
    assert all(ld % 8 == 0 and ld >= V for V in DC.LSE_V for ld in DC.lse_lds(V))
    assert {DC.lse_kernel_of(k, dt) for k in DC.LSE_K for dt in DC.DTYPES} == {k for k in DC.KERNELS if k.startswith("row_lse_topk")}
    assert set(DC.BIASES) == {0.0, -1e7, -3.5, 2.0}
    x, _ = DC.lse_edge_rows(16389)
    assert (x[0] == 12.0).sum() == 40 and np.isfinite(x[2]).sum() < 8 and np.isneginf(x[3, :8192]).all() and np.isfinite(x[3, 8192:]).all()
    assert all(set(DC.tiles_ntiles(k)) >= {1, k, k + 1, 255, 256, 257, 4096} for k in DC.TILES_K) and DC.tiles_V(4096) == 262144
    assert all(DC.tiles_V(n) % 64 for n in (1, 8, 255, 257))
    assert set(DC.WARP_V) == {1, 5, 1023, 1024, 1025, 2049, 5003} and all(set(DC.warp_ks(V)) >= {0, 1, V - 1, V, V + 5} for V in DC.WARP_V)
    assert {(R * V) % 2 for R in DC.SAMPLE_R for V in DC.SAMPLE_V} == {0, 1}
    bits = DC.warp_rows(1025, "f32")[2].astype(F).view(np.uint32)
    k = DR.okey(bits.view(F), canon=False)
    assert len({int(q) >> 21 for q in k[0::3]}) == 1 and len({int(q) >> 10 for q in k[1::3]}) == 1 and len(set(k[1::3].tolist())) > 100


def test_every_decode_instantiation_has_a_case_and_is_launched():
    ns = lambda s: re.sub(r"\s+", "", s)  # noqa: E731
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    built = {k for k in table["decode"] if any(fnmatch.fnmatchcase(k, p) for p in DC.PATTERNS)}
    assert len(built) == 16 and {ns(k) for k in built} == {ns(k) for k in DC.KERNELS}, sorted(built ^ set(DC.KERNELS))
    assert set(table["decode"]) - built == {"beam_step_kernel"}
    with open(os.path.join(ROOT, COVERAGE_PROFILE)) as f:
        traced = {ns(m) for m in re.findall(r"\b(?:row_lse_topk_kernel|row_topk_tiles_kernel|sample_rows_kernel|warp_threshold_kernel)<[^>]*>|\b(?:greedy_step_kernel|fill_i32_kernel)\b", f.read())}
    assert {ns(k) for k in DC.KERNELS} <= traced, sorted({ns(k) for k in DC.KERNELS} - traced)
