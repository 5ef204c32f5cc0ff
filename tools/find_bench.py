"""Record-find timing on config[4]'s world (workload.record_world: 500k players, each with a 64-row
skill record): "which rows of this player's skill record hold cooldown == 0" for n players at once

  (a) through nfk_find_rows (one call, one launch), and
  (b) the only way the C-ABI had before it: one nfk_get_records of the column's 64 rows per find
      (64 n cells in one call) and a numpy compare on the host,

in one process after 4 frames, for n = 1, 4096, 65 536 and 500 000.  Wall times are host clocks around
the whole call (each call ends in a stream synchronisation); (a)'s device time is the HIP-event time
around its launch (nfk_find_stats).  --rounds alternating rounds of the two paths per n; a round's figure
is the median of its repetitions, and the spread is the range of the rounds' figures.  (b) reads 0 for an
unused row, so its answer is masked with the used-row masks (read once, not timed) before the two
answers are compared — before anything is timed.  The kernel's bytes are the finds' descriptors (32),
used masks (8), used cells (8 per used row) and results (8).

usage: python tools/find_bench.py [--rounds 4] [--out profiles/record_find_500k.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noahgameframe_amd import kernel, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--n-obj", type=int, default=500_000)
    ap.add_argument("--sizes", default="1,4096,65536,500000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.record_world(n_ticks=4, n_obj=a.n_obj, groups=max(a.n_obj // 16, 1))
    m = kernel.world_from_workload(w)
    for t in range(4):
        kernel.run_workload(m, w, t, collect=False)
    m.synchronize()
    rows = int(w["rec_rows"][0])
    gh, gd = w["guid_head"], w["guid_data"]
    col, value = 1, np.uint64(0)   # the cooldown column (workload.programs: col 1); "which skills are ready"
    rng = np.random.default_rng(1)
    order = rng.permutation(a.n_obj)
    used_all = np.zeros(a.n_obj, np.uint64)
    m._chk(m.lib.nfk_get_used_rows(m.h, a.n_obj, kernel._p(gh), kernel._p(gd), kernel._p(np.zeros(a.n_obj, np.int32)),
                                   kernel._p(used_all)))
    weights = np.uint64(1) << np.arange(rows, dtype=np.uint64)
    with open(os.path.join(ROOT, "profiles", "hbm_ceiling.json")) as f:
        ceiling = json.load(f)["kernels"]["read_only"]["GBps"]
    st = {}
    lines = [f"record finds on config[4]'s world: {a.n_obj} objects, one {rows}-row record each "
             f"({int(np.mean([bin(int(x)).count('1') for x in used_all[:4096]]))} rows used on average); "
             f"{a.rounds} alternating rounds, a round = the median of its repetitions; median (min .. max of the rounds), ms"]
    ok = True
    for n in [min(int(x), a.n_obj) for x in a.sizes.split(",")]:
        o = np.sort(order[:n])
        ah, ad = np.ascontiguousarray(gh[o]), np.ascontiguousarray(gd[o])
        rec, cols, bits = np.zeros(n, np.int32), np.full(n, col, np.int32), np.full(n, value, np.uint64)
        bh, bd = np.repeat(ah, rows), np.repeat(ad, rows)
        brec, bcol = np.zeros(n * rows, np.int32), np.full(n * rows, col, np.int32)
        brow = np.tile(np.arange(rows, dtype=np.int32), n)

        def path_a():
            return m.find_rows(ah, ad, rec, cols, bits, stats=st)

        def path_b():
            cells = m.get_records(bh, bd, brec, brow, bcol).reshape(n, rows)
            return (cells == value).astype(np.uint64) @ weights

        ra, rb = path_a(), path_b() & used_all[o]
        assert np.array_equal(ra, rb), f"n={n}: the two paths disagree"
        hits = int(sum(bin(int(x)).count("1") for x in ra[:4096]))
        m.set_profiling(True)
        reps_a = 20 if n <= 4096 else (5 if n <= 65536 else 2)
        reps_b = 20 if n == 1 else (3 if n <= 4096 else 1)
        ta, tb, ka = [], [], []
        for _ in range(a.rounds):
            xa, xk = [], []
            for _ in range(reps_a):
                t0 = time.perf_counter()
                path_a()
                xa.append((time.perf_counter() - t0) * 1e3)
                xk.append(st["kernel_ms"])
            xb = []
            for _ in range(reps_b):
                t0 = time.perf_counter()
                path_b()
                xb.append((time.perf_counter() - t0) * 1e3)
            ta.append(float(np.median(xa)))
            ka.append(float(np.median(xk)))
            tb.append(float(np.median(xb)))
        m.set_profiling(False)
        nbytes = 48 * n + 8 * int(sum(bin(int(x)).count("1") for x in used_all[o]))
        gbps = nbytes / (np.median(ka) * 1e-3) / 1e9 if np.median(ka) > 0 else 0.0
        faster = max(ta) < min(tb)
        ok = ok and (faster or n < 4096)
        lines.append(
            "n = %-7d (a) nfk_find_rows: wall %.3f (%.3f .. %.3f)  kernel %.4f  %d bytes -> %.0f GB/s (%.1f%% of the %d GB/s read stream)"
            % (n, np.median(ta), min(ta), max(ta), np.median(ka), nbytes, gbps, 100 * gbps / ceiling, ceiling))
        lines.append(
            "            (b) nfk_get_records x %d + numpy compare: wall %.3f (%.3f .. %.3f)   (b) / (a) = %.1f   %s   hits in the first %d finds: %d"
            % (rows, np.median(tb), min(tb), max(tb), np.median(tb) / np.median(ta),
               "(a) faster in every round" if faster else "(a) NOT faster beyond the rounds' spread", min(n, 4096), hits))
    lines.append("(b) keeps the window's used-row masks cached after its first call (nfk_get_records' per-window cache): "
                 "its repetitions are its best case")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    m.close()
    assert ok, "nfk_find_rows is not faster than the nfk_get_records path at every n >= 4096"


if __name__ == "__main__":
    main()
