"""CPU companion of the scratch-poisoning suite (tests/util_poison.py): the poison patterns per dtype, the region logic, the contract
table against the recorded inventory of small models (tests/golden/poison_inventory_names.txt: every name the device suite's models
produce), and the comparison core against planted defects — a reader of a stale tail, an amax over the capacity, a REST region left
dirty, a NaN that only the poisoned side shows."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_poison as U  # noqa: E402

NAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poison_inventory_names.txt")
# tensors that only a step over several ranks allocates: no single-GPU model records them
MULTI_RANK_ONLY = ["reducer.stage.0", "reducer.stage.1"]


def recorded():
    with open(NAMES) as f:
        return [ln.strip() for ln in f if ln.strip()]


# ================================================================================================ patterns
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_float_patterns(dtype):
    t = torch.zeros(5, 7, dtype=dtype)
    U.poison_(t, U.NAN)
    assert torch.isnan(t).all()
    U.poison_(t, U.LOUD)
    f = t.float().reshape(-1)
    assert torch.isfinite(f).all() and (f.abs() >= 2.9e38).all() and (f[0::2] > 0).all() and (f[1::2] < 0).all()
    assert float(torch.finfo(dtype).max) > U.LOUD_F32


@pytest.mark.parametrize("dtype,top", [(torch.float8_e4m3fn, 448.0), (torch.float8_e5m2, 57344.0)])
def test_fp8_patterns(dtype, top):
    t = torch.zeros(4, 6, dtype=dtype)
    U.poison_(t, U.NAN)
    assert (t.view(torch.uint8) == 0x7F).all() and torch.isnan(t.float()).all()
    U.poison_(t, U.LOUD)
    f = t.float().reshape(-1)
    assert (f[0::2] == top).all() and (f[1::2] == -top).all()
    assert top == float(torch.finfo(dtype).max)


def test_integer_patterns_are_in_range_for_every_role():
    for dtype in (torch.int32, torch.int64, torch.uint8):
        t = torch.full((3, 4), 77, dtype=dtype)
        for how in U.PASSES:
            U.poison_(t, how)
            assert (t == 1).all()
    st = torch.full((6, 2), -5, dtype=torch.int64)
    U.poison_(st, U.NAN, "stats")
    assert (st[:, 0] == 0).all() and (st[:, 1] == U.LNSTATS_FILL).all()  # (sum, sum of squares): the variance read from it is positive
    roles = {r.int_role for r in U.RULES if r.int_role is not None}
    assert roles <= set(U.INT_ROLES) and all(U.INT_ROLES[r] for r in roles)
    for r in U.RULES:
        assert r.int_role is None or r.contract in (U.SCRATCH, U.REST), r.pattern


def test_a_column_range_is_poisoned_through_a_copy():
    cache = torch.zeros(3, 8, 4)
    U.poison_(cache[:, 5:], U.NAN)
    assert torch.isnan(cache[:, 5:]).all() and (cache[:, :5] == 0).all()
    c = {"k": [cache], "v": [torch.zeros(3, 8, 4)], "cache_index": 2}
    cache.zero_()
    U.poison_user_cache(c, U.LOUD)
    assert (cache[:, :3] == 0).all() and (cache[:, 3:].abs() > 1e38).all() and (c["v"][0][:, 3:].abs() > 1e38).all()


# ================================================================================================ regions
def _covers(regions, rows):
    seen = np.zeros(rows, dtype=int)
    for rg in regions:
        seen[rg.index[0]] += 1
    return (seen == 1).all()


def test_pad_rows_regions():
    rule = U.classify("buf:d.hf")
    rg = U.regions_of((128, 16), rule, {"rows": 96})
    assert [(r.contract, r.index[0].start, r.index[0].stop, r.rest) for r in rg] == [(U.SCRATCH, 0, 96, None), (U.REST, 96, None, 0)]
    assert _covers(rg, 128)
    assert [r.contract for r in U.regions_of((128, 16), rule, {"rows": 128})] == [U.SCRATCH]
    assert [r.contract for r in U.regions_of((128, 16), U.classify("buf:d0.stats"), {"rows": 6})] == [U.SCRATCH, U.REST]


def test_slot_shortlist_and_workspace_regions():
    rg = U.regions_of((1024, 2), U.classify("f8.a_state"), {"slots": 40})
    assert [(r.contract, r.rest) for r in rg] == [(U.STATE, None), (U.REST, 0)] and _covers(rg, 1024)
    rg = U.regions_of((128, 8), U.classify("shortlist.E"), {"Ns": 41})
    assert [(r.contract, r.index[0].start) for r in rg] == [(U.STATE, 0), (U.REST, 41)] and _covers(rg, 128)
    V = 10
    rg = U.regions_of((3 * V + 1 + 5,), U.classify("trainer.det_ws"), {"vocab": V})
    assert [(r.contract, r.rest) for r in rg] == [(U.REST, U.INT_MAX), (U.REST, 0), (U.REST, -1), (U.REST, 0), (U.SCRATCH, None)]
    assert _covers(rg, 3 * V + 6)
    assert [(r.contract, r.rest) for r in U.regions_of((4,), U.classify("store.m"), {})] == [(U.STATE, None)]


def test_poison_touches_scratch_regions_only_and_rest_is_asserted():
    t = torch.zeros(128, 4)
    e = U.Entry("buf:d.hf", t, U.classify("buf:d.hf"), {"rows": 96})
    w = U.Entry("store.master", torch.ones(8), U.classify("store.master"))
    assert U.poison([e, w], U.NAN) == {}
    assert torch.isnan(t[:96]).all() and (t[96:] == 0).all() and (w.tensor == 1).all()
    U.assert_rest([e, w])
    t[100, 2] = 1e-30  # a kernel that wrote a padding row
    with pytest.raises(U.PoisonError, match="buf:d.hf"):
        U.assert_rest([e, w], "planted")
    ws = torch.tensor([U.INT_MAX] * 3 + [0] * 3 + [-1] * 3 + [0, 9, 9], dtype=torch.int32)
    d = U.Entry("trainer.det_ws", ws, U.classify("trainer.det_ws"), {"vocab": 3})
    U.assert_rest([d])
    U.poison([d], U.LOUD)
    assert ws.tolist()[:10] == [U.INT_MAX] * 3 + [0] * 3 + [-1] * 3 + [0] and ws.tolist()[10:] == [1, 1]
    ws[4] = 2  # a count the kernels did not restore
    with pytest.raises(U.PoisonError):
        U.assert_rest([d])


def test_scenario_state_is_left_alone():
    kv = torch.zeros(128, 4)
    e = U.Entry("buf:g.ckv0", kv, U.classify("buf:g.ckv0"), {"rows": 40})
    left = U.poison([e], U.NAN, scenario="decode")
    assert list(left) == ["buf:g.ckv0"] and (kv == 0).all()
    assert U.poison([e], U.NAN) == {} and torch.isnan(kv[:40]).all()


# ================================================================================================ the table
def test_every_recorded_name_has_exactly_one_contract_and_every_pattern_is_used():
    names = recorded() + MULTI_RANK_ONLY
    assert len(names) > 150
    used = set()
    for n in names:
        used.add(U.classify(n).pattern)  # raises unless exactly one pattern matches
    unused = [r.pattern for r in U.RULES if r.pattern not in used]
    assert not unused, f"patterns that match nothing a model produces: {unused}"


def test_the_table_has_no_catch_all():
    probes = ["buf:brand.new", "vec:brand.new", "buf:d.new", "buf:d0.new", "buf:v0.new", "buf:db.new", "buf:g.new", "vec:ce.new",
              "f8.new", "store.new", "trainer.new", "plan.beam.new", "plan.beam.sub.new", "shortlist.new", "lnf.dec0.qkv.new",
              "reducer.new", "buf:", "", "x", "buf:f8.new.q8", "buf:d0.qkv.y.q8"]
    for p in probes:
        with pytest.raises(U.PoisonError):
            U.classify(p)
    for r in U.RULES:
        assert r.reason.strip() and r.contract in (U.SCRATCH, U.REST, U.STATE)
        assert not any(tok in r.pattern for tok in (".*", ".+")), f"{r.pattern}: an open-ended pattern"


def _fake_model():
    bufs = {("d.hf", 96, 8, torch.float32): torch.zeros(128, 8), ("ce.loss", 1, torch.float32): torch.zeros(1), "ones_i32": torch.ones(16, dtype=torch.int32)}
    eng = SimpleNamespace(_bufs=bufs, f8=None, _lnf={})
    st = SimpleNamespace(master=torch.ones(32), lp=None, grad=torch.zeros(32), acc=None, m=None, v=None)
    st.lp = st.master
    m = SimpleNamespace(engine=eng, store=st)
    return m


def test_inventory_walk_and_an_unclassified_buffer():
    m = _fake_model()
    inv = U.inventory(m)
    assert sorted(e.name for e in inv) == ["buf:d.hf", "buf:ones_i32", "store.grad", "store.master", "vec:ce.loss"]
    assert U.names(m) == sorted(e.name for e in inv)
    m.engine._bufs[("brand.new", 4, 4, torch.float32)] = torch.zeros(128, 4)
    with pytest.raises(U.PoisonError, match="brand.new"):
        U.inventory(m)


# ================================================================================================ planted defects
ROWS, CAP, COLS = 40, 96, 8


class _Toy:
    """a toy engine with the defects planted: one row-padded buffer [128][COLS] of capacity CAP that every call fills up to `rows`"""

    def __init__(self, defect=None):
        self.defect = defect
        self.x = torch.zeros(128, COLS)
        self.entry = U.Entry("buf:d.hf", self.x, U.classify("buf:d.hf"), {"rows": CAP})

    def call(self, data):
        rows = data.shape[0]
        self.x[:rows] = data
        n_sum = CAP if self.defect == "stale_tail" else rows
        n_max = CAP if self.defect == "amax_cap" else rows
        if self.defect == "dirty_rest":
            self.x[CAP + 3] = 1.0
        # (the amax as the device computes it: fmax ignores NaN, like v_max_f32 and an atomic max on the bits)
        amax = torch.from_numpy(np.fmax.reduce(np.abs(self.x[:n_max].numpy()), axis=None, keepdims=True).reshape(1))
        return {"colsum": self.x[:n_sum].sum(0), "amax": amax}


def _history(defect, how):
    g = torch.Generator().manual_seed(3)
    first, second = torch.randn(CAP, COLS, generator=g), torch.randn(ROWS, COLS, generator=g)
    A, B, F = _Toy(defect), _Toy(defect), _Toy(defect)
    A.call(first), B.call(first)
    U.poison([A.entry], how)
    return A, A.call(second), B.call(second), F.call(second)


@pytest.mark.parametrize("how", U.PASSES)
def test_a_sound_toy_passes(how):
    A, got, twin, fresh = _history(None, how)
    U.compare(got, twin, (), "twin")
    U.compare(got, fresh, (), "fresh")
    U.assert_rest([A.entry])


def test_a_reader_of_a_stale_tail_is_caught_by_both_passes_and_by_the_fresh_model_alone_without_poison():
    for how in U.PASSES:
        A, got, twin, fresh = _history("stale_tail", how)
        with pytest.raises(U.PoisonError, match="colsum"):
            U.compare(got, twin, (), how)
    g = torch.Generator().manual_seed(3)
    first, second = torch.randn(CAP, COLS, generator=g), torch.randn(ROWS, COLS, generator=g)
    A, B, F = _Toy("stale_tail"), _Toy("stale_tail"), _Toy("stale_tail")
    A.call(first), B.call(first)
    got, twin, fresh = A.call(second), B.call(second), F.call(second)
    U.compare(got, twin, (), "a twin with the same history agrees: without poison it sees nothing")
    with pytest.raises(U.PoisonError):
        U.compare(got, fresh, (), "shape history against a fresh model")


def test_an_amax_over_the_capacity_hides_under_nan_and_shows_under_loud_values():
    A, got, twin, fresh = _history("amax_cap", U.NAN)
    U.compare(got, twin, (), "NaN pass: a max swallows NaN")  # (this is why there are two passes)
    A, got, twin, fresh = _history("amax_cap", U.LOUD)
    with pytest.raises(U.PoisonError, match="amax"):
        U.compare(got, twin, (), "loud pass")


def test_a_rest_region_left_dirty_is_caught():
    A, got, twin, fresh = _history("dirty_rest", U.NAN)
    U.compare(got, twin, (), "outputs agree")
    with pytest.raises(U.PoisonError, match="REST"):
        U.assert_rest([A.entry], "after the call")


def test_the_comparison_core():
    a = {"x": torch.tensor([1.0, 2.0, float("nan")]), "g": torch.tensor([1.0, -4.0])}
    b = {k: v.clone() for k, v in a.items()}
    U.compare(a, b, (), "NaN where the twin holds NaN too is no finding")
    c = {k: v.clone() for k, v in a.items()}
    c["x"][0] = float("nan")
    with pytest.raises(U.PoisonError, match="NaN / Inf"):
        U.compare(c, b, ("x",), "a NaN only the poisoned side shows, even on an atomically summed leaf")
    c = {k: v.clone() for k, v in a.items()}
    c["g"][0] = torch.tensor(1.0).view(torch.int32).add(1).view(torch.float32)
    with pytest.raises(U.PoisonError, match="bit for bit"):
        U.compare(c, b, (), "one ulp")
    U.compare(c, b, ("g",), "one ulp on an atomically summed leaf")
    c["g"][0] = 1.0 + 2.1 * U.ATOMIC_TOL * 4.0  # the bound is 2e-4 x the leaf's maximum (4)
    with pytest.raises(U.PoisonError, match="atomically"):
        U.compare(c, b, ("g",), "beyond the summation-order bound")
    c["g"][0] = 1.0 + 0.9 * U.ATOMIC_TOL * 4.0
    U.compare(c, b, ("g",), "inside it")
    with pytest.raises(U.PoisonError, match="kind"):
        U.compare({"x": a["x"]}, b, (), "a missing output")
    z = {"s": torch.tensor([0.0])}
    with pytest.raises(U.PoisonError):
        U.compare({"s": torch.tensor([-0.0])}, z, (), "signed zero is a bit")
    i = {"ids": torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)}
    with pytest.raises(U.PoisonError, match="ids"):
        U.compare({"ids": torch.tensor([[1, 2], [3, 5]], dtype=torch.int32)}, i, (), "token ids")


def test_copy_state_moves_state_only():
    a, b = _fake_model(), _fake_model()
    a.store.master.fill_(3.0)
    a.store.grad.fill_(7.0)
    U.copy_state(U.inventory(a), U.inventory(b))
    assert (b.store.master == 3.0).all() and (b.store.grad == 0).all()
