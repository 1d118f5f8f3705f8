"""Reference for mic_beam_step / mic_beam_step_groups: a numpy restatement of one beam_search_body_fn iteration (gen:857-966, the
lines of oracle.generation_ref.beam_search) that starts from what the kernel is given — the per-row top-2K candidates instead of the
logits — plus the loop condition (gen:798-820) as the kernel keeps it on the device (gstate).  fp32 arithmetic in the oracle's
operation order, one batch item at a time; the two length-penalty divisors are inputs, so a test can move them by ulps.

`defect=` seeds the mistakes the suite has to reject (tests/test_beam_conformance_cpu.py); None is the design."""
import math
from collections import Counter

import numpy as np

F = np.float32
NEG = F(-1.0e7)  # gen:764, 766, 811, 890, 919
STATE = ("running_seq", "running_scores", "seq", "scores", "finished", "src_row", "next_token", "flags")
INT_STATE = ("running_seq", "seq", "finished", "src_row", "next_token", "flags")
DEFECTS = ("slot_ties", "merge_new_wins", "no_full", "neg_before_div", "src_from_new", "ticket_all", "stride_128")


# ------------------------------------------------------------------------------------------------ length penalty
def ulps(x, j):
    """the fp32 value j ulp away from x"""
    x = F(x)
    for _ in range(abs(int(j))):
        x = np.nextafter(x, F(np.inf if j > 0 else -np.inf), dtype=F)
    return x


def divisors(cur_len, L, lp):
    """(div_cur, div_L) = fl32(pow64(cur_len, fl32(lp))), fl32(pow64(L, fl32(lp))): the divisors of gen:910 and gen:805-807.

    The oracle forms div_cur in fp32 (numpy's fp32 pow, which equals this for every cur_len in 1..128 and the lp values used here) and
    div_L from the Python double lp.  mic_beam_step_args carries length_penalty as a float, so fl32(lp) is all the kernel can know: div_L
    is taken with fl32(lp) too.  For an lp that fp32 holds exactly the two readings coincide; for lp = 1.2 they may differ by one ulp of
    div_L, which can only touch the `improve` flag (oracle_div_L gives the oracle's reading)."""
    lp32 = float(F(lp))
    return F(math.pow(float(cur_len), lp32)), F(math.pow(float(L), lp32))


def oracle_div_L(L, lp):
    """gen:805-807 as oracle.generation_ref.beam_search reads it: the exponent is the Python double"""
    return F(float(L) ** float(lp))


# ------------------------------------------------------------------------------------------------ state
def init_state(items, K, L, start, pad):
    """the state a beam search starts from (gen:751-766) for `items` batch items; src_row: every row owns its slot 0"""
    R = items * K
    s = {"running_seq": np.full((items, K, L), pad, np.int32), "seq": np.full((items, K, L), pad, np.int32),
         "finished": np.zeros((items, K), np.int32), "scores": np.full((items, K), NEG, F),
         "running_scores": np.tile(np.array([0.0] + [NEG] * (K - 1), F), (items, 1)), "next_token": np.full(R, start, np.int32),
         "src_row": np.zeros((R, L), np.int32), "flags": np.zeros((items, 2), np.int32)}
    s["running_seq"][:, :, 0] = start
    s["src_row"][:, 0] = np.arange(R, dtype=np.int32)
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def _desc(val, idx):
    """positions ordered (value descending, idx ascending)"""
    return np.lexsort((idx, -val.astype(np.float64)))


def improve_of(best_running_score, scores, finished, div_L):
    """gen:805-815 for one item: every worst_finished strictly below best_running"""
    best_running = F(best_running_score) / F(div_L)
    worst = np.where(finished != 0, scores.min(), NEG)
    return int(np.all(worst < best_running))


def step_ref(state, cand_val, cand_idx, K, L, V, cur_len, eos, div_cur, div_L, early_stopping, defect=None, stats=None):
    """One launch over every item of `state` (arrays as in mic_beam_step_args: running_seq / seq [B][K][L], running_scores / scores /
    finished [B][K], src_row [B*K][L], next_token [B*K], flags [B][2]); cand_val fp32 / cand_idx int [B*K][2K].
    Returns (new state, flags); flags is new_state["flags"] = per item {all finished, can still improve}."""
    C = 2 * K
    B = state["scores"].shape[0]
    new = copy_state(state)
    cand_val = np.asarray(cand_val, F).reshape(B * K, C)
    cand_idx = np.asarray(cand_idx, np.int64).reshape(B * K, C)
    div_cur, div_L = F(div_cur), F(div_L)
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        val, tok = cand_val[rows].reshape(-1), cand_idx[rows].reshape(-1)
        beam = np.repeat(np.arange(K), C)
        flat = beam * V + tok                                      # gen:859: index into the [K * V] row of the item
        if defect == "slot_ties":
            flat = np.arange(K * C)
        o = _desc(val, flat)
        if stats is not None and K * C > C and val[o[C - 1]] == val[o[C]]:
            stats["top2k_cut_tie"] += 1
        o = o[:C]                                                  # gen:872-873
        if defect == "stride_128" and K >= 9:                      # pairs past the first 128 never rank themselves in
            keep = o < 128
            topk_lp = np.where(keep, val[o], NEG).astype(F)
            topk_beam = np.where(keep, beam[o], 0)
            topk_tok = np.where(keep, tok[o], 0)
        else:
            topk_lp, topk_beam, topk_tok = val[o].astype(F), beam[o], tok[o]   # gen:874
        old_run, old_seq = state["running_seq"][b], state["seq"][b]
        old_scores, old_fin = state["scores"][b], state["finished"][b]
        topk_seq = old_run[topk_beam].copy()                       # gen:875-877
        topk_seq[:, cur_len] = topk_tok                            # gen:878-881
        just_fin = topk_tok == eos                                 # gen:889
        topk_lp = (topk_lp + just_fin.astype(F) * NEG).astype(F)   # gen:890
        on = _desc(topk_lp, np.arange(C))
        if stats is not None and topk_lp[on[K - 1]] == topk_lp[on[K]]:
            stats["next_cut_tie"] += 1
        nxt = on[:K][::-1]                                         # gen:895-897
        all_fin_old = bool((old_fin != 0).all())
        full = all_fin_old and bool(early_stopping) and defect != "no_full"   # gen:911-917
        add_pen = ((~just_fin) | full).astype(F)                   # gen:918
        if defect == "neg_before_div":
            fs = ((topk_lp + add_pen * NEG).astype(F) / div_cur).astype(F)
        else:
            fs = (topk_lp / div_cur).astype(F)                     # gen:910
            fs = (fs + add_pen * NEG).astype(F)                    # gen:919
        merged = np.concatenate([old_scores.astype(F), fs])        # gen:928
        mkey = np.arange(K + C)
        if defect == "merge_new_wins":
            mkey = (mkey - K) % (K + C)
        om = _desc(merged, mkey)
        mi = om[:K][::-1]                                          # gen:932-934
        merged_seq = np.concatenate([old_seq, topk_seq], axis=0)   # gen:925-927
        merged_fin = np.concatenate([old_fin != 0, just_fin])      # gen:929-931
        if stats is not None:
            for p in range(K):                                     # ties that decide a slot of the selection
                if p + 1 < K + C and merged[om[p]] == merged[om[p + 1]]:
                    a_old, b_old = om[p] < K, om[p + 1] < K
                    if a_old != b_old:
                        stats["merge_tie_old_new"] += 1
                        break
            for p in range(K):
                if p + 1 < K + C and merged[om[p]] == merged[om[p + 1]] and om[p] >= K and om[p + 1] >= K:
                    stats["merge_tie_new_new"] += 1
                    break
            if full:
                stats["full"] += 1
            if all_fin_old and not early_stopping and bool((merged_fin[mi] & (mi >= K)).any()):
                stats["late_admit"] += 1
        new["running_seq"][b] = topk_seq[nxt]                      # gen:898-903
        new["running_scores"][b] = topk_lp[nxt]
        new["seq"][b] = merged_seq[mi]                             # gen:935-940
        new["scores"][b] = merged[mi]
        new["finished"][b] = merged_fin[mi].astype(np.int32)
        new["next_token"][rows] = topk_tok[nxt]
        parent = topk_beam[nxt]                                    # gen:945-953: row nb continues the cache of row `parent`
        src = state["src_row"][rows][np.arange(K) if defect == "src_from_new" else parent].copy()
        src[:, cur_len] = b * K + np.arange(K)                     # and owns the slot of the token it feeds next
        new["src_row"][rows] = src
        new["flags"][b, 0] = int(new["finished"][b].all())         # gen:818
        new["flags"][b, 1] = improve_of(new["running_scores"][b, K - 1], new["scores"][b], new["finished"][b], div_L)
    return new, new["flags"]


# ------------------------------------------------------------------------------------------------ loop state
def search_stop(flags, cur_len, L, early_stopping):
    """beam_search_cond_fn (gen:798-820) negated, over the items of one search: (stop, the terms that hold)"""
    flags = np.asarray(flags).reshape(-1, 2)
    terms = {"stop_all_finished": bool(flags[:, 0].all()) and bool(early_stopping), "stop_no_improve": not bool(flags[:, 1].all()),
             "stop_length": cur_len + 1 >= L}
    return any(terms.values()), terms


class gstate_ref:
    """gs[3] (done) and gs[4] (steps) of each of G searches; gs[0..2] (counters and ticket) are zero after every launch"""

    def __init__(self, G):
        self.done, self.steps = [0] * G, [0] * G

    def live(self, g):
        return not self.done[g]

    def launch(self, g, stop):
        self.steps[g] += 1
        self.done[g] = int(bool(stop))

    def array(self):
        a = np.zeros((len(self.done), 8), np.int64)
        a[:, 3], a[:, 4] = self.done, self.steps
        return a


# ------------------------------------------------------------------------------------------------ grouped launches
def of_group(x, g, G, K, per_row):
    """rows (per_row) or items of search g out of an item-major array of a G-search launch (item i belongs to search i % G)"""
    n = K if per_row else 1
    x = np.asarray(x)
    per = x.shape[0] // (G * n)
    return x.reshape(per, G, n, *x.shape[1:])[:, g].reshape(per * n, *x.shape[1:])


def local_rows(src, G, K):
    """a row id of the grouped launch (item * K + beam) as the search's own run numbers it ((item // G) * K + beam)"""
    return (src // K // G) * K + src % K


def split_state(s, G, K):
    """the state of a G-search launch as G single-search states"""
    out = []
    for g in range(G):
        t = {}
        for name in STATE:
            per_row = name in ("src_row", "next_token")
            x = s[name]
            v = of_group(x if per_row else x.reshape(x.shape[0], -1), g, G, K, per_row)
            if name == "src_row":
                v = local_rows(v, G, K)
            if not per_row:
                v = v.reshape(-1, *s[name].shape[1:])
            t[name] = np.ascontiguousarray(v)
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ the fake cache
class FakeCache:
    """fed[row][pos] = the token the row fed at `pos` (slot index = position of the fed token).  A beam that inherits its parent's
    history through src_row must find its own running sequence in the slots it points at."""

    def __init__(self, rows, L, start):
        self.fed = np.full((rows, L), -1, np.int64)
        self.fed[:, 0] = start

    def feed(self, next_token, cur_len, rows=None):
        rows = np.arange(self.fed.shape[0]) if rows is None else rows
        self.fed[rows, cur_len] = np.asarray(next_token)[rows]

    def check(self, src_row, running_seq, cur_len, what, rows=None):
        src_row = np.asarray(src_row)
        run = np.asarray(running_seq).reshape(src_row.shape)
        rows = np.arange(src_row.shape[0]) if rows is None else rows
        for pos in range(cur_len + 1):
            got = self.fed[src_row[rows, pos], pos]
            assert np.array_equal(got, run[rows, pos]), f"{what}: cache slot {pos}: rows read {got.tolist()}, sequences hold {run[rows, pos].tolist()}"


# ------------------------------------------------------------------------------------------------ a whole case
class RefRun:
    """The reference trajectory of a case of tests/util_beam_cases.py, launch by launch.  The G searches of a grouped launch run
    separately on their de-interleaved items.  launch(n) returns one entry per search: (state after the launch, done, steps, stepped);
    shift = (j_cur, j_L) moves the two divisors of that launch by ulps; commit=False leaves the run where it was."""

    def __init__(self, case, defect=None, stats=None, div_L_of=None):
        self.case, self.defect, self.div_L_of = case, defect, div_L_of
        self.stats = stats if stats is not None else Counter()
        self.G = case["G"] or 1
        self.states = split_state(case["state"], self.G, case["K"])
        self.gs = gstate_ref(self.G)
        self.launches = launches_of(case)

    def launch(self, n, shift=(0, 0), commit=True):
        c, G = self.case, self.G
        K, L, V, lp, early = c["K"], c["L"], c["V"], c["lp"], c["early"]
        cur_len, val, idx = self.launches[n]
        div_cur, div_L = divisors(cur_len, L, lp)
        if self.div_L_of is not None:
            div_L = self.div_L_of(L, lp)
        div_cur, div_L = ulps(div_cur, shift[0]), ulps(div_L, shift[1])
        stats = self.stats if commit else Counter()
        states, gs = list(self.states), gstate_ref(G)
        gs.done, gs.steps = list(self.gs.done), list(self.gs.steps)
        live = [g for g in range(G) if gs.live(g)]
        for g in live:
            states[g], _ = step_ref(states[g], of_group(val, g, G, K, True), of_group(idx, g, G, K, True), K, L, V, cur_len, c["eos"],
                                    div_cur, div_L, early, defect=self.defect, stats=stats)
        every = np.concatenate([states[g]["flags"] for g in range(G)])
        stops = []
        for g in live:
            stop, terms = search_stop(every if self.defect == "ticket_all" else states[g]["flags"], cur_len, L, early)
            stops.append(stop)
            gs.launch(g, stop)
            if stop:
                for t, holds in terms.items():
                    stats[t] += int(holds)
        if G > 1 and any(stops) and not all(gs.done):
            stats["group_stops_alone"] += 1
        if commit:
            self.states, self.gs = states, gs
        return [(states[g], gs.done[g], gs.steps[g], g in live) for g in range(G)]


def run_ref(case, defect=None, stats=None, div_L_of=None):
    """every launch of the case: a list of RefRun.launch results"""
    r = RefRun(case, defect, stats, div_L_of)
    return [r.launch(n) for n in range(len(r.launches))]


def launches_of(case):
    """the launches a runner makes: the case's own until every search has ended (at most all of them), then two more that repeat the
    last one's arguments — decided by the reference, which `run_ref` and the GPU runner share through case["n_launches"]"""
    ls = case["launches"]
    n = case.get("n_launches")
    if n is None:
        return list(ls)
    return [ls[min(i, len(ls) - 1)] for i in range(n)]


def plan_launches(case):
    """sets case["n_launches"]: the launches up to the one at which the last search ends, plus two"""
    case.pop("n_launches", None)
    traj = run_ref(case)
    n = len(traj)
    for i, per in enumerate(traj):
        if all(done for _, done, _, _ in per):
            n = i + 3
            break
    case["n_launches"] = n
    return case


def int_outputs(per):
    """what must not move when the divisors move by ulps: every integer array, done and steps of every search after one launch"""
    return [tuple(s[name].tobytes() for name in INT_STATE) + (done, steps) for s, done, steps, _ in per]
