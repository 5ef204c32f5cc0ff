"""Scene-query timing on config[1]'s world (workload.bench_world: 1M objects in one scene, 32,768
players): GetObjectByProperty on Level over the scene's players

  (a) through nfk_query_objects (one query, and a batch of 16 queries on 16 values), and
  (b) the best answer the C-ABI allowed before it: one batched nfk_get_props of every player's Level
      and a numpy filter on the host,

in one process after 4 frames.  Wall times are host clocks around the whole call (each call ends in a
stream synchronisation), medians of --reps repetitions after --warmup unrecorded ones, the two paths
alternating; (a)'s device time is the HIP-event time around its launches (nfk_query_result.kernel_ms).
The two answers are compared before anything is timed.

usage: python tools/query_bench.py [--reps 50] [--warmup 5] [--out profiles/scene_query_1M.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noahgameframe_amd import kernel, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-obj", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.bench_world(n_obj=a.n_obj, groups=max(a.n_obj // 256, 1), n_ticks=4)
    m = kernel.world_from_workload(w)
    for t in range(4):
        kernel.run_workload(m, w, t, collect=False)
    m.synchronize()
    lv = workload.PID["Level"]
    gh, gd = w["guid_head"], w["guid_data"]
    players = np.nonzero(w["is_player"])[0]
    # the players in the reference's order (one scene: group, then NFGUID)
    players = players[np.lexsort((gd[players], gh[players], w["group"][players]))]
    ph, pd, pp = np.ascontiguousarray(gh[players]), np.ascontiguousarray(gd[players]), np.full(len(players), lv, np.int32)
    values = list(range(20, 36))

    def path_a(vals):
        return m.query_objects([kernel.query(1, pid=lv, value=v) for v in vals], stats=st)

    def path_b(v):
        got = m.get_props(ph, pd, pp).view(np.int64)
        # (nfk_get_props caches its device reads for the window: dropped by the next frame only, so
        #  every repetition but the first answers from the host cache — the parent's best case)
        return players[got.astype(np.int32) == v]

    st = {}
    ra, rb = path_a(values[:1])[0], path_b(values[0])
    assert ra.tolist() == rb.tolist() and len(ra) > 0, "the two paths disagree"
    m.set_profiling(True)
    t_a1, t_a16, t_b, k_a1, k_a16 = [], [], [], [], []
    for i in range(a.warmup + a.reps):
        rec = i >= a.warmup
        t0 = time.perf_counter()
        path_a(values[:1])
        t1 = time.perf_counter()
        k1 = st["kernel_ms"]
        b1 = st["bytes"]
        path_a(values)
        t2 = time.perf_counter()
        k16 = st["kernel_ms"]
        b16 = st["bytes"]
        path_b(values[0])
        t3 = time.perf_counter()
        if rec:
            t_a1.append((t1 - t0) * 1e3)
            t_a16.append((t2 - t1) * 1e3)
            t_b.append((t3 - t2) * 1e3)
            k_a1.append(k1)
            k_a16.append(k16)
    # (b) without the window's read cache: one cold call after a frame
    m.ExecuteCalls()
    m.synchronize()
    t0 = time.perf_counter()
    path_b(values[0])
    b_cold = (time.perf_counter() - t0) * 1e3
    med = lambda x: float(np.median(x))
    spread = lambda x: (float(np.percentile(x, 10)), float(np.percentile(x, 90)))
    lines = [
        f"scene queries on config[1]'s world: {a.n_obj} objects, one scene, {len(players)} players, "
        f"{m.outputs()['n_tiles']} tiles; {a.reps} repetitions after {a.warmup} warm-up, medians (p10 .. p90), ms",
        f"hits of Level == {values[0]}: {len(ra)}",
        "(a)  nfk_query_objects, 1 query:    wall %.3f (%.3f .. %.3f)   kernels %.3f   read back %d bytes"
        % (med(t_a1), *spread(t_a1), med(k_a1), b1),
        "(a)  nfk_query_objects, 16 queries: wall %.3f (%.3f .. %.3f)   kernels %.3f   read back %d bytes"
        % (med(t_a16), *spread(t_a16), med(k_a16), b16),
        "(b)  nfk_get_props of the scene's players + numpy filter: wall %.3f (%.3f .. %.3f)" % (med(t_b), *spread(t_b)),
        "(b)  the same, first call of a window (no cached reads): wall %.3f (one call)" % b_cold,
        "ratio (b) / (a), 1 query: %.1f;  16 queries / 16 x 1 query: %.2f" % (med(t_b) / med(t_a1),
                                                                         med(t_a16) / (16 * med(t_a1))),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    assert med(t_a1) < med(t_b), "nfk_query_objects is not faster than the batched get_props path"
    m.close()


if __name__ == "__main__":
    main()
