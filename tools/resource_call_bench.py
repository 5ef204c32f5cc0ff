"""Resource-call timing on config[1]'s world (workload.bench_world: 1,048,576 objects): n AddHP-shaped
calls (NFK_ADJ_GAIN_ALIVE on HP against MAXHP) on n distinct objects in a clean window

  (a) through nfk_adjust_props (one call, one launch), and
  (b) the only route the C-ABI had before it: two batched nfk_get_props (HP, MAXHP), the rule in numpy,
      then nfk_set_props of the accepted calls,

in one process after 2 frames, for n = 1, 4096, 65 536 and 1 048 576.  Wall times are host clocks around
the whole call (each ends in a stream synchronisation); (a)'s device time is the HIP-event time around
its launch (nfk_adjust_stats).  Every timed repetition runs in a clean window: an untimed frame after it
applies the queued Sets (after a batch its (object, dst) pairs are pending, and both routes would then be
answered from the host's overlay).  --rounds alternating rounds of the two routes per n; a round's figure
is the median of its repetitions, and the spread is the range of the rounds' figures.  Before anything is
timed the new call's values are compared with the rule over the values read before it.  The kernel's bytes are
the calls' descriptors (40), the two cells read (16) and the results (9).  A report, not a gate.

usage: python tools/resource_call_bench.py [--rounds 4] [--out profiles/resource_calls_1M.txt]
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

HP, MAXHP = workload.PID["HP"], workload.PID["MAXHP"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--n-obj", type=int, default=1 << 20)
    ap.add_argument("--sizes", default="1,4096,65536,1048576")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.bench_world(n_obj=a.n_obj, groups=max(a.n_obj // 256, 1), n_ticks=4)
    m = kernel.world_from_workload(w)
    now = [int(w["tick_time"][0])]

    def frame():
        now[0] += 100
        m.Execute(now[0])
        m.synchronize()
    frame()
    frame()
    gh, gd = w["guid_head"], w["guid_data"]
    rng = np.random.default_rng(1)
    order = rng.permutation(a.n_obj)
    with open(os.path.join(ROOT, "profiles", "hbm_ceiling.json")) as f:
        ceiling = json.load(f)["kernels"]["read_only"]["GBps"]
    st = {}
    lines = [f"resource calls on config[1]'s world: {a.n_obj} objects; n AddHP-shaped calls on distinct objects, clean windows; "
             f"{a.rounds} alternating rounds, a round = the median of its repetitions; median (min .. max of the rounds), ms"]
    for n in [min(int(x), a.n_obj) for x in a.sizes.split(",")]:
        o = np.sort(order[:n])
        ah, ad = np.ascontiguousarray(gh[o]), np.ascontiguousarray(gd[o])
        op = np.full(n, kernel.ADJ_GAIN_ALIVE, np.uint8)
        dst, bound, v = np.full(n, HP, np.int32), np.full(n, MAXHP, np.int32), np.full(n, 25, np.int64)

        def path_a():
            return m.adjust_props(ah, ad, op, dst, bound, v, stats=st)

        def path_b():
            cur = m.get_props(ah, ad, dst).view(np.int64)
            mx = m.get_props(ah, ad, bound).view(np.int64)
            ret = (v > 0).astype(np.uint8)
            hit = (v > 0) & (cur > 0)
            m.set_props(ah[hit], ad[hit], dst[hit], np.minimum(cur[hit] + v[hit], mx[hit]).view(np.uint64))
            return ret | (hit.astype(np.uint8) << 1)

        # the two routes agree: results, and the values a read sees afterwards
        pre, mx = m.get_props(ah, ad, dst).view(np.int64), m.get_props(ah, ad, bound).view(np.int64)
        ra = path_a()
        va = m.get_props(ah, ad, dst).view(np.int64)
        assert st["n_host"] == 0 and int(((ra & 2) != 0).sum()) == st["n_set"]
        assert np.array_equal(va, np.where(pre > 0, np.minimum(pre + 25, mx), pre)), f"n={n}: nfk_adjust_props' values"
        frame()
        rb = path_b()   # (another window: HP has moved, so only the return values compare)
        assert np.array_equal(ra & 1, rb & 1), f"n={n}: the two routes' return values differ"
        frame()
        m.set_profiling(True)
        reps = 10 if n <= 4096 else (4 if n <= 65536 else 2)
        ta, tb, ka = [], [], []
        for _ in range(a.rounds):
            xa, xk, xb = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                path_a()
                xa.append((time.perf_counter() - t0) * 1e3)
                xk.append(st["kernel_ms"])
                assert st["n_host"] == 0 and st["n_dev"] == n
                frame()
            for _ in range(reps):
                t0 = time.perf_counter()
                path_b()
                xb.append((time.perf_counter() - t0) * 1e3)
                frame()
            ta.append(float(np.median(xa)))
            ka.append(float(np.median(xk)))
            tb.append(float(np.median(xb)))
        m.set_profiling(False)
        nbytes = 65 * n
        gbps = nbytes / (np.median(ka) * 1e-3) / 1e9 if np.median(ka) > 0 else 0.0
        verdict = ("(a) faster in every round" if max(ta) < min(tb) else
                   "(a) SLOWER in every round" if min(ta) > max(tb) else "no difference beyond the rounds' spread")
        lines.append("n = %-7d (a) nfk_adjust_props: wall %.3f (%.3f .. %.3f)  kernel %.4f  %d bytes -> %.0f GB/s (%.1f%% of the %d GB/s read stream)"
                     % (n, np.median(ta), min(ta), max(ta), np.median(ka), nbytes, gbps, 100 * gbps / ceiling, ceiling))
        lines.append("            (b) 2 x nfk_get_props + numpy + nfk_set_props: wall %.3f (%.3f .. %.3f)   (b) / (a) = %.2f   %s"
                     % (np.median(tb), min(tb), max(tb), np.median(tb) / np.median(ta), verdict))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    m.close()


if __name__ == "__main__":
    main()
