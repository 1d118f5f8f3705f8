"""Beam-step conformance on the MI355X: mic_beam_step and mic_beam_step_groups (csrc/decode.hip, beam_step_kernel) on every case of
tests/util_beam_cases.py against the numpy restatement of one beam_search_body_fn iteration in tests/util_beam_ref.py, which
tests/test_beam_conformance_cpu.py ties to oracle.generation_ref.beam_search.  One test per (K, G, length-penalty group); per case:
  - every state array, flags, next_token and gstate is a window in a canary-filled allocation; canaries and the candidate inputs
    keep their bits;
  - after every launch every integer array equals the reference, running_scores and scores are bit-equal to it (-inf included),
    gs[3] (done) and gs[4] (steps) equal gstate_ref and gs[0..2] are zero; search g of a G-search launch is compared with the
    reference run on its de-interleaved items (src_row renumbered);
  - the fake cache: fed[src_row[row][pos]][pos] == running_seq[row][pos] for every row and pos <= cur_len;
  - the two launches after the last search has ended change no byte of any output;
  - the whole chain runs twice from refilled buffers and gives identical bits after every launch.
Length penalties that go through pow (lp not in {0, 1}): bit-equality as well, against the reference with the divisors
fl32(pow64(cur_len, fl32(lp))) and fl32(pow64(max_len, fl32(lp))).  The kernel used to take both from device powf; measured against
this suite on the MI355X that was one ulp off at 13 ** 0.5 (+1), 9 ** 0.75 and 10 ** 0.75 (+1), 3 ** 1.25 (+1), 9 ** 1.2 and
12 ** 1.2 (-1), 10 ** 1.2 (+1) — the largest distance |j_cur| = 1, j_L = 0 wherever it showed, and 0 at lp in {0, 1} — so the
launcher now computes both on the host in double and the distance allowed is 0 for every lp.  The cases stay admissible (no integer
output depends on the last two ulps of a divisor, tests/test_beam_conformance_cpu.py): a score that misses says by how many ulps of
which divisor, and the test prints the (j_cur, j_L) it found per (cur_len, lp) — all (0, 0) on the MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_beam_cases as BC  # noqa: E402
import util_beam_ref as BR  # noqa: E402
from test_attn_conformance_gpu import Buf  # noqa: E402
from test_decode_conformance_gpu import IBuf, refused  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHIFTS = sorted(((jc, jl) for jc in range(-BC.MAX_ULP, BC.MAX_ULP + 1) for jl in range(-BC.MAX_ULP, BC.MAX_ULP + 1)),
                key=lambda j: (max(abs(j[0]), abs(j[1])), abs(j[0]) + abs(j[1]), j))
FLOATS = ("running_scores", "scores")


class _Bufs:
    """the arguments of one case on the device"""

    def __init__(self, c, dev):
        K, L, items = c["K"], c["L"], c["items"]
        R, C = items * K, 2 * K
        self.c = c
        self.out = {"running_seq": IBuf(R, L, dev), "seq": IBuf(R, L, dev), "finished": IBuf(items, K, dev), "src_row": IBuf(R, L, dev),
                    "next_token": IBuf(1, R, dev), "flags": IBuf(items, 2, dev), "gstate": IBuf(c["G"] or 1, 8, dev),
                    "running_scores": Buf(items, K, K, F32, dev, "canary", off=4), "scores": Buf(items, K, K, F32, dev, "canary", off=4)}
        self.val, self.idx = Buf(R, C, C, F32, dev, "canary", off=4), IBuf(R, C, dev)
        self.forced = IBuf(1, R, dev)

    def start(self):
        for b in list(self.out.values()) + [self.val, self.idx, self.forced]:
            b.refill()
        for name, x in self.c["state"].items():
            self.out[name].put(x.reshape(self.out[name].rows, -1))
        self.out["gstate"].put(np.zeros((self.c["G"] or 1, 8)))

    def f32(self, name):
        return self.out[name].t.contiguous().cpu().numpy()

    def state(self):
        c = self.c
        s = {name: (self.f32(name) if name in FLOATS else self.out[name].get().astype(np.int32)) for name in BR.STATE}
        s["running_seq"] = s["running_seq"].reshape(c["items"], c["K"], c["L"])
        s["seq"] = s["seq"].reshape(c["items"], c["K"], c["L"])
        s["next_token"] = s["next_token"].reshape(-1)
        return s

    def bits(self):
        return [b.bits() for b in self.out.values()]


def _launch(ops, b, n):
    """launch n of the case: the candidates keep their bits, every canary of every argument too"""
    c = b.c
    cur_len, val, idx = BR.launches_of(c)[n]
    R, C = c["items"] * c["K"], 2 * c["K"]
    what = f"{c['name']} launch {n}"
    if n in c.get("forced", {}) and n < len(c["launches"]):
        # the candidates of a forced first step come from mic_row_forced_topk itself (bias: the running scores on the device)
        b.val.refill()
        b.idx.refill()
        b.forced.put(c["forced"][n].reshape(1, R))
        ops.row_forced_topk(R, C, b.forced.t, b.val.t, b.idx.t, row_bias=b.out["running_scores"].t)
        torch.cuda.synchronize()
        assert np.array_equal(b.val.t.cpu().numpy().view(np.int32), val.view(np.int32)), f"{what}: mic_row_forced_topk values"
        assert np.array_equal(b.idx.get(), idx), f"{what}: mic_row_forced_topk indices"
    else:
        b.val.t.copy_(torch.from_numpy(val))
        b.idx.put(idx)
    before = (b.val.bits(), b.idx.bits())
    o = b.out
    ops.beam_step(c["items"], c["K"], c["L"], c["V"], cur_len, c["eos"], c["pad"], c["lp"], c["early"], b.val.t, b.idx.t, o["running_seq"].t,
                  o["running_scores"].t, o["seq"].t, o["scores"].t, o["finished"].t, o["src_row"].t, o["next_token"].t, o["flags"].t,
                  gstate=o["gstate"].t, groups=c["G"])
    torch.cuda.synchronize()
    assert torch.equal(b.val.bits(), before[0]) and torch.equal(b.idx.bits(), before[1]), f"{what}: the candidates were written"
    b.val.check_canary(what)
    b.idx.check_canary(what)
    for name, x in o.items():
        x.check_canary(f"{what} {name}")


def _matches(got, gs, per):
    """the device state against the reference of every search: (integers equal, floats bit-equal, the first difference)"""
    ints, floats, first = True, True, None
    for g, (s, done, steps, _) in enumerate(per):
        for name in BR.STATE:
            if name in FLOATS:
                ok = np.array_equal(got[g][name].view(np.int32), s[name].view(np.int32))
                floats &= ok
            else:
                ok = np.array_equal(got[g][name], s[name])
                ints &= ok
            if not ok and first is None:
                first = f"search {g}: {name}: got {got[g][name].reshape(-1)[:12].tolist()} ..., reference {s[name].reshape(-1)[:12].tolist()} ..."
        if (int(gs[g, 3]), int(gs[g, 4])) != (done, steps):
            ints, first = False, first or f"search {g}: gs[3], gs[4] = {gs[g, 3]}, {gs[g, 4]}, reference {done}, {steps}"
        if gs[g, :3].any() or gs[g, 5:].any():
            ints, first = False, first or f"search {g}: gstate {gs[g].tolist()}"
    return ints, floats, first


def _run_case(ops, c, dev, dist):
    K, L, G = c["K"], c["L"], c["G"] or 1
    b = _Bufs(c, dev)
    n_launches = c["n_launches"]
    first_run = None
    for rerun in range(2):
        b.start()
        ref = BR.RefRun(c)
        cache = BR.FakeCache(c["items"] * K, L, BC.START)
        first_len = c["launches"][0][0]
        cache.fed[:, :first_len] = c["state"]["running_seq"].reshape(-1, L)[:, :first_len]   # (every row of a starting state owns its slots)
        snaps = []
        for n in range(n_launches):
            cur_len = ref.launches[n][0]
            what = f"{c['name']} launch {n} (cur_len {cur_len})"
            _launch(ops, b, n)
            snaps.append(b.bits())
            if rerun:
                assert all(torch.equal(x, y) for x, y in zip(snaps[n], first_run[n])), f"{what}: two runs of the chain differ"
                continue
            got_all = b.state()
            got, gs = BR.split_state(got_all, G, K), b.out["gstate"].get()
            found = None
            for j in SHIFTS:   # (0, 0) first; the others only say how far off a score that misses is
                ints, floats, why = _matches(got, gs, ref.launch(n, shift=j, commit=False))
                if j == (0, 0):
                    assert ints, f"{what}: {why}"
                    why0 = why
                if ints and floats:
                    found = j
                    break
            assert found == (0, 0), f"{what}: {why0} (the divisors (div_cur, div_L) that give these scores: {found} ulp away)"
            per = ref.launch(n)
            stepped = [g for g in range(G) if per[g][3]]
            if stepped:
                dist.setdefault((cur_len, c["lp"]), set()).add(found)
                rows = np.concatenate([(np.arange(c["items"])[g::G][:, None] * K + np.arange(K)).reshape(-1) for g in stepped])
                cache.feed(got_all["next_token"], cur_len, rows)
                cache.check(got_all["src_row"], got_all["running_seq"], cur_len, what, rows)
            else:
                assert all(torch.equal(x, y) for x, y in zip(snaps[n], snaps[n - 1])), f"{what}: a launch after the end wrote something"
        first_run = first_run or snaps


@pytest.mark.parametrize("K,G,group", BC.PARAMS, ids=[f"K{K}-G{G}-{group}" for K, G, group in BC.PARAMS])
def test_beam_step(dev, K, G, group):
    from mic_amd import ops

    dist = {}
    for c in BC.cases(K, G, group):
        _run_case(ops, c, dev, dist)
    worst = 0
    for (cur_len, lp), js in sorted(dist.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        for jc, jl in sorted(js):
            worst = max(worst, abs(jc), abs(jl))
        if group == "pow":
            print(f"[conformance] beam_step K={K} G={G} lp={lp} cur_len={cur_len}: (j_cur, j_L) = {sorted(js)}")
    print(f"[conformance] beam_step K={K} G={G} {group}: largest |j| {worst} over {len(dist)} (cur_len, lp) pairs")
    assert worst == 0


def test_beam_step_refusals(dev):
    """bad shapes, an LDS request over 65 536 B, a null pointer, a group count that does not divide B: refused on the host, nothing
    written, and mic_last_error names the entry point"""
    from mic_amd import ops

    c = BC.base(3, 8, 61, 4, 2, 1.0, True, "refusals")
    b = _Bufs(c, dev)
    b.start()
    val, idx = BC.candidates(4, 3, 61, 1, 1, [99] * 4)[0]
    b.val.t.copy_(torch.from_numpy(val))
    b.idx.put(idx)
    o = b.out
    outs = list(o.values())

    def call(B=4, K=3, L=8, cur_len=2, groups=None, **null):
        a = {name: (None if name in null else x.t) for name, x in o.items()}
        v, i = (None if "cand_val" in null else b.val.t), (None if "cand_idx" in null else b.idx.t)
        return lambda: ops.beam_step(B, K, L, 61, cur_len, BC.EOS, BC.PAD, 1.0, True, v, i, a["running_seq"], a["running_scores"], a["seq"],
                                     a["scores"], a["finished"], a["src_row"], a["next_token"], a["flags"], gstate=a["gstate"], groups=groups)

    for groups in (None, 2):
        for what, kw in (("K = 33", dict(K=33)), ("K = 0", dict(K=0)), ("max_len = 1", dict(L=1, cur_len=1)), ("cur_len = 0", dict(cur_len=0)),
                         ("cur_len = max_len", dict(cur_len=8)), ("K = 32 with L = 163", dict(K=32, L=163)), ("null cand_val", dict(cand_val=1)),
                         ("null src_row", dict(src_row=1)), ("null flags", dict(flags=1))):
            refused(call(groups=groups, **kw), outs, f"{what} groups={groups}", "mic_beam_step")
    refused(call(groups=3), outs, "B % groups != 0", "mic_beam_step_groups")
    refused(call(groups=0), outs, "groups = 0", "mic_beam_step_groups")
    refused(call(B=0, groups=2), outs, "B = 0", "mic_beam_step_groups")
