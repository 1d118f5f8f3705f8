"""Writes tests/golden/gemm_plan_parent.npz: a sweep of mic_gemm_plan over drawn argument sets, recorded on the commit BEFORE the
GEMM dispatch decision moved into one host function (run it on a checkout of that commit with its library built; it is kept for
the record, the fixture is not meant to be regenerated on later commits).  tests/test_gemm_plan_equivalence_cpu.py replays the
draws on the current library and asks for the identical return code and legacy report fields.

The drawn inputs are stored next to the answers (layout: tests/util_gemm_cases.py), so nothing depends on a random generator
reproducing them.  Every draw passes mic_gemm's host checks (fill_epi / launch_bf16; include/mic_hip.h): split_k > 1 only with a
bare fp32 C (fp8: NT slabs), rowstat only with the bare bias epilogue of an NT launch with an aligned bf16 C and N % 64 == 0, fp8
operands in the same layout with K % 128 == 0, k-major operands with M / N multiples of 8 (fp8: 16), an fp8 C only behind an
activation / dact epilogue of an NT launch.

The draws stay where that commit's report and that commit's launcher agree; the places where they do not are pinned by named
tests on the launcher's side instead (tests/test_gemm_plan_equivalence_cpu.py):
  - split_k <= K / 64 (fp8: K / 128): the report took "not PLAIN" from the unclamped split_k, the launch from the clamped one;
  - rowstat on a single bf16 NT problem with N % 128 != 0 comes with K an odd multiple of 64, which keeps the launch off
    gemm_d2.hip (K % 128 != 0): the launcher gave such a launch with K % 128 == 0 to gemm_d2 (256 x 128 tiles), the report wanted
    N % 128 == 0 for that and answered with the 256 x 256 tiling;
  - under MIC_GEMM_D2=2 the single bf16 NT problems reported with 256 x 256 tiles are left out: that switch moved them to gemm_d2
    at launch, and the report did not know;
  - no folded LayerNorm and no operand of 2 GiB or more (with softmax partials the launcher keeps both off gemm_d2, the report
    did not look).
One block of draws at the default switches, one per entry of util_gemm_cases.SWITCHES; the switches latch at the first GEMM
call, so each block is recorded in a child process."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import util_gemm_cases as GC  # noqa: E402

N_DEFAULT, N_SWITCH = 5200, 340
PRODUCT_DIMS = (768, 1024, 2404, 2432, 3072, 3200, 4096)
COMBOS = ((256, 256, 1, 1, 0), (256, 256, 1, 1, 1), (256, 256, 1, 1, 2), (128, 256, 1, 2, 2), (128, 192, 1, 2, 0), (128, 128, 1, 2, 0),
          (128, 128, 2, 1, 0), (64, 64, 4, 1, 0), (64, 64, 2, 2, 0), (64, 64, 1, 4, 0))  # (tile, tile_m, kgroups, blocks_per_cu, phased)


def _dim(rng, align):
    u = rng.random()
    v = (rng.integers(1, 513) if u < 0.3 else rng.integers(513, 4097) if u < 0.6 else rng.choice(PRODUCT_DIMS) if u < 0.87
         else 16384 if u < 0.95 else GC.V_PAD)
    return int(-(-int(v) // align) * align)


def draw(rng):
    """-> (dtype, akm, bkm, cus, [problem rows])"""
    dt = int(rng.choice(3, p=(0.6, 0.2, 0.2)))
    akm, bkm = ((0, 0), (0, 1), (1, 1))[rng.choice(3, p=(0.5, 0.25, 0.25))] if dt == 0 else ((0, 0), (1, 1))[rng.choice(2, p=(0.7, 0.3))]
    count = int(rng.choice((1, 2, 3, 8), p=(0.7, 0.12, 0.1, 0.08)))
    cus = int(rng.choice((0, 248, 192, 128, 64), p=(0.5, 0.125, 0.125, 0.125, 0.125)))
    nt = not akm and not bkm
    # (softmax partials want every problem of their launch on the bare epilogue: a group carries them on all problems or on none)
    rowstat = nt and rng.random() < (0.12 if count == 1 else 0.2)
    probs = []
    for _ in range(count):
        al = 16 if dt and akm else 8
        M, N = _dim(rng, al if akm else 1), _dim(rng, al if bkm else 1)
        if max(M, N) > 100000:
            M, N = (M, min(N, 4096)) if M > N else (min(M, 4096), N)
        kq = 128 if dt else 64
        K = int(rng.choice((1024, 2432 // kq * kq, 3200 // kq * kq, 16384))) if rng.random() < 0.2 else kq * int(rng.integers(1, 4096 // kq + 1))
        if max(M, N) > 100000:
            K = min(K, 2432 // kq * kq)
        fl, actid, split, c8 = 0, 0, 0, 0
        ldc_pad = int(rng.choice((0, 8, 3), p=(0.4, 0.4, 0.2)))
        u = rng.random()
        if rowstat:  # softmax partials: bare bias epilogue, bf16 C, N % 64 == 0, aligned C
            N = -(-N // 64) * 64
            if rng.random() < 0.5:
                N = (N // 128) * 128 + (64 if rng.random() < 0.5 else 128)
            fl, ldc_pad = GC.F_BIAS | GC.F_ROWSTAT, int(rng.choice((0, 8)))
            if dt == 0 and count == 1 and N % 128 and K % 128 == 0:
                K += 64  # (see the module docstring: where the report and the launcher of that commit disagree)
        elif u < 0.17 and (dt == 0 or nt):  # split-K: raw fp32 partial sums, atomics or (fp8: only) slabs
            fl = GC.F_C32
            ok = [s for s in (2, 6) if s <= K // kq]
            if ok:
                split = int(rng.choice(ok))
                if dt or rng.random() < 0.5:
                    fl |= GC.F_SLABS
        elif u < 0.27 and dt and nt:  # fp8 C: emitted behind an activation / dact epilogue, vector path only
            N, ldc_pad, c8 = -(-N // 8) * 8, int(rng.choice((0, 8))), 1 + int(rng.integers(0, 2))
            actid = int(rng.integers(1, 4))
            fl = GC.F_DACT if rng.random() < 0.4 else (GC.F_BIAS | (GC.F_ZOUT if rng.random() < 0.6 else 0))
        else:
            fl = (GC.F_C32 if rng.random() < 0.3 else 0) | (GC.F_BIAS if rng.random() < 0.5 else 0)
            v = rng.random()
            if v < 0.3:
                actid, fl = int(rng.integers(1, 4)), fl | (GC.F_ZOUT if rng.random() < 0.6 else 0)
            elif v < 0.45:
                actid, fl = int(rng.integers(1, 4)), fl | GC.F_DACT
            fl |= (GC.F_RES if rng.random() < 0.25 else 0) | (GC.F_ACC if rng.random() < 0.2 else 0) | (GC.F_OFF if rng.random() < 0.12 else 0)
            if akm and dt == 0 and rng.random() < 0.4:
                fl |= GC.F_ROWSUM
        probs.append([M, N, K, N + ldc_pad, fl, actid, split, c8])
    return dt, akm, bkm, cus, probs


def record_block(path, block):
    fx = np.load(path)
    rows = np.nonzero(fx["draws"][:, 6] == block)[0]
    np.save(path + f".{block}.npy", np.array(GC.plan_answers(fx["draws"], fx["probs"], rows), np.int32))


def main():
    rng = np.random.default_rng(20261016)
    draws, probs = [], []
    for block in range(len(GC.SWITCHES) + 1):
        # (the MIC_GEMM_D2=2 block loses the draws named in the module docstring afterwards)
        n = N_DEFAULT if block == 0 else (N_SWITCH * 2 if GC.SWITCHES[block - 1][:2] == ("MIC_GEMM_D2", "2") else N_SWITCH)
        for _ in range(n):
            dt, akm, bkm, cus, ps = draw(rng)
            draws.append([len(probs), len(ps), dt, akm, bkm, cus, block])
            probs += ps
    draws, probs = np.array(draws, np.int32), np.array(probs, np.int32)
    answers = np.zeros((len(draws), 1 + len(GC.ANSWER_FIELDS)), np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "draws.npz")
        np.savez(path, draws=draws, probs=probs)
        for block in range(len(GC.SWITCHES) + 1):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MIC_")]:
                del env[k]
            if block:
                env[GC.SWITCHES[block - 1][0]] = GC.SWITCHES[block - 1][1]
            subprocess.run([sys.executable, os.path.abspath(__file__), "--block", path, str(block)], env=env, check=True)
            answers[draws[:, 6] == block] = np.load(path + f".{block}.npy")
    f = {k: i + 1 for i, k in enumerate(GC.ANSWER_FIELDS)}
    keep = np.ones(len(draws), bool)
    for block, (env, val, _) in enumerate(GC.SWITCHES, 1):
        if (env, val) == ("MIC_GEMM_D2", "2"):
            keep &= ~((draws[:, 6] == block) & (draws[:, 2] == 0) & (draws[:, 3] == 0) & (draws[:, 4] == 0) & (draws[:, 1] == 1) &
                      (answers[:, f["tile"]] == 256))
    draws, answers = draws[keep], answers[keep]
    # the conditions of the sweep, checked here on the recording commit: they are about the inputs, not about the code under test
    assert (answers[:, 0] == 0).all()
    per_block = np.bincount(draws[:, 6], minlength=len(GC.SWITCHES) + 1)
    assert per_block[0] >= 5000 and (per_block[1:] >= 300).all(), per_block
    d0 = answers[draws[:, 6] == 0]
    combos = {}
    for a in d0:
        key = tuple(int(a[f[k]]) for k in ("tile", "tile_m", "kgroups", "blocks_per_cu", "phased"))
        combos[key] = combos.get(key, 0) + 1
    assert set(combos) == set(COMBOS) and min(combos.values()) >= 20, combos
    assert {1, 2, 3, 8} <= set(draws[:, 1].tolist()) and set(draws[:, 5].tolist()) == {0, 248, 192, 128, 64}
    out = os.path.join(HERE, os.path.basename(GC.PLAN_FIXTURE))
    np.savez_compressed(out, draws=draws, probs=probs, answers=answers)
    print(f"{out}: {len(draws)} draws {per_block.tolist()}, {len(probs)} problems, {os.path.getsize(out)} bytes; default-switch plans:")
    for k in COMBOS:
        print("  ", k, combos[k])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--block"]:
        record_block(sys.argv[2], int(sys.argv[3]))
    else:
        main()
