"""The cases of the beam-step conformance suite (tests/test_beam_conformance_cpu.py, tests/test_beam_conformance_gpu.py).

Every candidate value and every hand-built score sits on the grid of multiples of 1/4 in [-40, 0], so every fp32 add is exact or a
plain round-to-nearest and ties are exact by construction.  EOS = 2, PAD = 1, start token 5.

A case is a dict: K, L, V, items, G (None: mic_beam_step; an int: mic_beam_step_groups with item i in search i % G), lp, early, eos,
pad, state (the arrays of mic_beam_step_args before the first launch), launches [(cur_len, cand_val [items*K][2K] fp32, cand_idx
int32)], n_launches (the launches up to the one that ends the last search, plus two that must change nothing).  forced {launch:
token per row}: the candidates of that launch are mic_row_forced_topk's for these tokens with the state's running scores as the
bias — stored here from that kernel's reference (util_decode_ref.forced_ref), produced by the kernel itself in the GPU test."""
import functools

import numpy as np

import util_beam_ref as BR
import util_decode_ref as DR

F = np.float32
EOS, PAD, START = 2, 1, 5
KS = (1, 2, 3, 8, 9, 16, 17, 32)
LS = (2, 14)
VS = (61, 250054)
LAYOUTS = ((1, None), (1, 1), (5, None), (5, 1), (5, 5))      # (items, G)
GS = (None, 1, 5)
LP_EXACT = (0.0, 1.0)                                          # device pow must give the divisor exactly: no distance allowed
LP_POW = (0.5, 0.75, 1.25, 2.0, 1.2)                           # every one but 1.2 is exact in fp32
GROUPS = {"exact": LP_EXACT, "pow": LP_POW}
MAX_ULP = 2                                                    # the range over which a "pow" case must be admissible


def candidates(items, K, V, steps, seed, finish_at):
    """per step ([items*K, 2K] fp32 values, int32 tokens): values from a coarse grid (ties within and across rows), sorted per row
    like the output of the top-k kernels; distinct tokens per row in random order (so a tie inside a row is not in token order), an
    EOS here and there; from step finish_at[item] on every row of that item leads with EOS, above every other candidate of the item:
    the item collects K finished hypotheses at that step."""
    rng = np.random.RandomState(seed)
    R, C = items * K, 2 * K
    out = []
    for t in range(1, steps + 1):
        val = -np.sort(t + rng.randint(0, 6, (R, C)) / 4.0, axis=1)
        if V - 4 <= 4096:
            idx = np.argsort(rng.rand(R, V - 4), axis=1)[:, :C] + 4
        else:
            idx = rng.randint(4, V, (R, C))
            idx[0, 0] = V - 1                                  # the far end of the vocabulary, in the first beam and the last
            idx[R - 1, C - 1] = V - 1
            for r in range(R):
                while np.unique(idx[r]).size != C:
                    idx[r] = rng.randint(4, V, C)
        rare = rng.rand(R) < 0.05
        slot = rng.randint(0, C, R)
        idx[rare, slot[rare]] = EOS
        for i in range(items):
            if t >= finish_at[i]:
                rows = slice(i * K, (i + 1) * K)
                sub = idx[rows]
                sub[sub == EOS] = 3                            # (3 is never drawn above: tokens stay distinct within a row)
                sub[:, 0] = EOS
                val[rows, 0] += 2.0
        out.append((val.astype(F), idx.astype(np.int32)))
    return out


def base(K, L, V, items, G, lp, early, name):
    return dict(name=name, K=K, L=L, V=V, items=items, G=G, lp=lp, early=early, eos=EOS, pad=PAD,
                state=BR.init_state(items, K, L, START, PAD), launches=[])


def admissible(case):
    """no integer output of any launch moves when div_cur and div_L move independently by up to MAX_ULP ulp (checked along the
    reference trajectory): the scores may then differ by ulps without any decision depending on it"""
    if case["lp"] in LP_EXACT:
        return True
    r = BR.RefRun(case)
    js = range(-MAX_ULP, MAX_ULP + 1)
    for n in range(len(r.launches)):
        want = BR.int_outputs(r.launch(n, commit=False))
        cur_len = r.launches[n][0]
        _, div_L = BR.divisors(cur_len, case["L"], case["lp"])
        for jc in js:
            per = r.launch(n, shift=(jc, 0), commit=False)
            if BR.int_outputs(per) != want:
                return False
            for s, _, _, stepped in per:                       # div_L enters through `improve` alone
                if stepped:
                    for b in range(s["scores"].shape[0]):
                        for jl in js:
                            if BR.improve_of(s["running_scores"][b, -1], s["scores"][b], s["finished"][b], BR.ulps(div_L, jl)) != s["flags"][b, 1]:
                                return False
        r.launch(n)
    return True


def _finish_at(items, G, L, k):
    """items of one search fill their finished beams at different steps (k rotates the schedule); with G = items every search has one
    item and ends at a step of its own; the last entry never finishes"""
    sched = [3, 5, 4, 7, 99]
    return [sched[(i + k) % 5] for i in range(items)]


def chain(K, L, V, items, G, lp, early, k):
    """a search from the initial state; regenerated (next seed) until admissible"""
    for attempt in range(50):
        c = base(K, L, V, items, G, lp, early, f"chain K={K} L={L} V={V} items={items} G={G} lp={lp} early={int(early)}")
        seed = 1000 * k + 17 * K + L + items + (G or 0) + 100003 * attempt
        c["launches"] = [(t, v, i) for t, (v, i) in enumerate(candidates(items, K, V, L - 1, seed, _finish_at(items, G, L, k)), start=1)]
        BR.plan_launches(c)
        if admissible(c):
            return c
    raise AssertionError("no admissible chain")


def _cand(K, rows, tok0=40):
    """rows: per row a list of (value, token), best first; padded to 2K with low distinct candidates (tokens from tok0)"""
    C = 2 * K
    val, idx = np.zeros((len(rows), C), F), np.zeros((len(rows), C), np.int32)
    for r, row in enumerate(rows):
        row = list(row) + [(-38.0 - 0.25 * (j % 8), tok0 + j) for j in range(C - len(row))]
        val[r], idx[r] = [v for v, _ in row], [t for _, t in row]
    return val, idx


def _mid_state(items, K, L, cur_len, fin_scores=None):
    """a state `cur_len` tokens into a search: beam k of item i has written the tokens 10 + i + k, 11 + i + k, ...; every row owns its
    own cache slots; fin_scores[i] (ascending, best last): the item's finished beams hold these scores (None: none finished)"""
    s = BR.init_state(items, K, L, START, PAD)
    for i in range(items):
        for k in range(K):
            s["running_seq"][i, k, 1:cur_len] = 10 + i + k + np.arange(cur_len - 1)
            s["src_row"][i * K + k, :cur_len] = i * K + k
            s["running_scores"][i, k] = -cur_len - 0.25 * (K - 1 - k)
        if fin_scores is not None and fin_scores[i] is not None:
            s["scores"][i] = fin_scores[i]
            s["finished"][i] = 1
            for k in range(K):
                s["seq"][i, k, 1:cur_len - 1] = 20 + i + k + np.arange(cur_len - 2)
                s["seq"][i, k, cur_len - 1] = EOS
    return s


@functools.lru_cache(maxsize=None)
def single_steps(group):
    """launches from hand-built states.  A finished hypothesis scores (value - 1e7) / cur_len ** lp (gen:890 comes before gen:910), so
    the hand-built finished scores are of that size"""
    out = []
    if group == "exact":
        for early in (True, False):
            # every beam of item 0 finished; item 1 keeps the search alive.  EOS candidates that beat the old finished scores
            # ((-1 - 1e7) / 4 against -2.8e6): early stopping penalises them (`full`), without it they enter
            K, L, cur = 3, 8, 4
            c = base(K, L, 61, 2, None, 1.0, early, f"all beams finished early={int(early)}")
            c["state"] = _mid_state(2, K, L, cur, [[-3.0e6, -2.9e6, -2.8e6], None])
            rows = [[(-1.0, EOS), (-4.0, 7)], [(-2.0, EOS), (-4.25, 8)], [(-4.0, 9), (-4.5, EOS)]] + [[(-4.0, 11)], [(-4.25, 12)], [(-4.5, 13)]]
            c["launches"] = [(cur, *_cand(K, rows))]
            out.append(c)
        for G in (None, 1):
            # a new finished candidate whose score equals an old finished score bit for bit ((-3 - 1e7) / 2 = -5000001.5, at the cut of
            # the merge): the old one stays
            K, L, cur = 2, 8, 2
            c = base(K, L, 61, 1, G, 1.0, False, f"merge tie old against new G={G}")
            c["state"] = _mid_state(1, K, L, cur, [[-5000001.5, -5000000.5]])
            c["launches"] = [(cur, *_cand(K, [[(-3.0, EOS), (-3.25, 7)], [(-3.5, 8)]]))]
            out.append(c)
            # equal values across beams with the same token: the lower beam ranks first (flat index beam * V + token), at the cut of
            # the top-2K, among the next running beams and among the finished candidates
            K, L, cur = 3, 8, 3
            c = base(K, L, 61, 1, G, 1.0, True, f"same token across beams G={G}")
            c["state"] = _mid_state(1, K, L, cur)
            c["launches"] = [(cur, *_cand(K, [[(-3.0, 7), (-3.0, EOS), (-3.25, 9)]] * 3))]
            out.append(c)
        for K, items, G in ((3, 2, None), (9, 5, 5)):
            # the first step of generate() with a forced language token: one finite candidate per row (0 + the running score: 0 in
            # beam 0, -1e7 in the others), the rest -inf with the lowest indices that skip the forced one
            V = 250054
            c = base(K, 8, V, items, G, 1.0, True, f"-inf tails of the forced step K={K}")
            forced = np.repeat(np.array([250004, 0, 17, V - 1, 3][:items], np.int32), K)
            C, bias = 2 * K, c["state"]["running_scores"].reshape(-1)
            v, i = np.zeros((forced.size, C), F), np.zeros((forced.size, C), np.int32)
            for r in range(forced.size):
                v[r], i[r] = DR.forced_ref(V, int(forced[r]), C, float(bias[r]))
            c["forced"] = {0: forced}    # launch 0: the GPU test takes these candidates from mic_row_forced_topk
            c["launches"] = [(1, v, i)] + [(t, cv, ci) for t, (cv, ci) in enumerate(candidates(items, K, V, 3, 7 + K, [99] * items), start=1)][1:]
            out.append(c)
        # cur_len = L - 1: nothing finished, everything can improve, the stop is by length alone
        K, L = 3, 6
        c = base(K, L, 61, 2, None, 1.0, True, "last step")
        c["state"] = _mid_state(2, K, L, L - 1)
        c["launches"] = [(L - 1, *candidates(2, K, 61, 1, 5, [99, 99])[0])]
        out.append(c)
        # worst_finished == best_running exactly (-1 against -8 / 8) at lp = 1: the comparison is strict, improve = 0 and the search
        # ends; a quarter more (-7.75 / 8) and it goes on.  (Finished scores this high need a hand-built state.)
        for K in KS:
            for early in (True, False):
                for top, tag in ((-8.0, "equal"), (-7.75, "above")):
                    L, cur = 8, 3
                    c = base(K, L, 250054, 2, None, 1.0, early, f"worst_finished against best_running: {tag} K={K} early={int(early)}")
                    c["state"] = _mid_state(2, K, L, cur, [[-1.0] + [-0.5] * (K - 1), None])
                    rows = [[(top, 7), (-9.0, 8)]] + [[(-9.0, 9 + k)] for k in range(1, K)] + [[(-9.0, 9 + k)] for k in range(K)]
                    c["launches"] = [(cur, *_cand(K, rows, tok0=100))]
                    out.append(c)
        # K = 32 at L = 162: the largest LDS request the launcher accepts (65 280 B), at the last four positions of the sequences
        K, L, V = 32, 162, 250054
        c = base(K, L, V, 5, None, 1.0, True, "K=32 L=162")
        c["state"] = _mid_state(5, K, L, 158)
        c["launches"] = [(157 + t, v, i) for t, (v, i) in enumerate(candidates(5, K, V, 4, 32162, [99, 3, 99, 2, 99]), start=1)]
        out.append(c)
    for c in out:
        BR.plan_launches(c)
    return out


@functools.lru_cache(maxsize=None)
def cases(K, G, group):
    """the cases of one test: per shape two chains whose (lp, early) rotate through the group's values, then the single steps"""
    out, lps = [], GROUPS[group]
    combos = [(lp, early) for lp in lps for early in (True, False)]
    k = KS.index(K) * 7 + GS.index(G) * 3
    for L in LS:
        for V in VS:
            if 2 * K > V:
                continue
            for items, g in LAYOUTS:
                if g != G:
                    continue
                for _ in range(2):
                    lp, early = combos[k % len(combos)]
                    out.append(chain(K, L, V, items, G, lp, early, k))
                    k += 1
    out += [c for c in single_steps(group) if c["K"] == K and c["G"] == G]
    return out


PARAMS = [(K, G, group) for K in KS for G in GS for group in GROUPS]


def all_cases():
    return [c for p in PARAMS for c in cases(*p)]
