"""Enter-snapshot timing: the OnPropertyEnter / OnRecordEnter payload of n objects at once

  (a) through nfk_snapshot_objects_obj (one call: k_snap count, k_snap_scan, k_snap write,
      k_snap_cells, one pinned copy back), and
  (b) the only way the C-ABI had before it: nfk_get_props for every int / f64 property of the view,
      nfk_get_objects for its object properties, nfk_get_used_rows and nfk_get_records of the used
      rows' cells for its record, then a numpy filter with the same predicates,

in one process after 4 frames: on config[1]'s world (workload.bench_world, 1M objects) n = 256 (one
group: a player's enter), 4 096, 65 536 and 1 048 576 in the public view; on config[4]'s world
(workload.record_world, 500k players with a 64-row record) n = 1, 4 096 and 500 000 in the private view.
Requests are in slot order (what nfk_query_objects returns).  Wall times are host clocks around the
whole call (each ends in a stream synchronisation); (a)'s device time is the HIP-event time around its
launches (kernel_ms, profiling on).  --rounds alternating rounds of the two paths per n; a round's
figure is the median of its repetitions, the spread is the range of the rounds' figures.  The two
answers are compared for equality before anything is timed.  The kernels' bytes as the tool counts
them: per request 8 (descriptor) + 8 per property word loaded + 20 per property entry written; per
record entry 24 (its mask and the written entry) + 16 per cell (read and write); set against
profiles/hbm_ceiling.json's read-write mix.  (a) must be faster than (b) in every round at n >= 4096.

usage: python tools/snapshot_bench.py [--rounds 4] [--out profiles/enter_snapshot_1M.txt]
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


def popcount(u):
    c = np.zeros(len(u), np.int64)
    for b in range(64):
        c += ((u >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return c


def bench(name, w, view, sizes, rounds, ceiling, emit):
    m = kernel.world_from_workload(w)
    for t in range(4):
        kernel.run_workload(m, w, t, collect=False)
    m.synchronize()
    n_obj = len(w["guid_head"])
    gh, gd, cls = w["guid_head"], w["guid_data"], np.asarray(w["cls"])
    n_int, n_flt = int(w["cfg"][1]), int(w["cfg"][2])
    n_if, n_op = n_int + n_flt, m.n_oprops
    flag = workload.PRIVATE if view == kernel.VIEW_PRIVATE else workload.PUBLIC
    pflags = np.asarray(w["prop_flags"])
    pids = np.array([p for p in range(n_if + n_op) if (pflags[:, p] & flag).any()], np.int32)
    n_rec = int(w["cfg"][5])
    rflags = np.asarray(w["rec_flags"]) if n_rec else np.zeros((len(pflags), 0), np.uint8)
    recs = [r for r in range(n_rec) if (rflags[:, r] & flag).any()]
    assert len(recs) <= 1, "path (b) of this tool handles one record in view"
    slots = np.concatenate(m.query_objects([kernel.query(1, who=kernel.Q_PLAYERS), kernel.query(1, who=kernel.Q_OTHERS)]))
    slots = np.sort(slots) if len(slots) != n_obj else slots
    rng = np.random.default_rng(1)
    emit(f"{name}: {n_obj} objects, view {'private' if flag == workload.PRIVATE else 'public'}: {len(pids)} properties "
         f"({int((pids >= n_if).sum())} object) and {len(recs)} record(s) in view; {rounds} alternating rounds, a round = "
         f"the median of its repetitions; median (min .. max of the rounds), ms")
    ok = True
    st = {}
    for n in [min(int(x), n_obj) for x in sizes]:
        start = int(rng.integers(0, n_obj - n + 1))
        o = np.ascontiguousarray(slots[start:start + n]).astype(np.int32)   # a run of the slot order
        views = np.full(n, view, np.uint8)
        ah, ad = np.ascontiguousarray(gh[o]), np.ascontiguousarray(gd[o])
        ip = pids[pids < n_if]
        op = pids[pids >= n_if]
        in_view = (pflags[cls[o]][:, pids] & flag) != 0                      # [n][K] by the object's class
        K = len(pids)
        bh_i, bd_i, bp_i = np.repeat(ah, len(ip)), np.repeat(ad, len(ip)), np.tile(ip, n)
        bh_o, bd_o, bp_o = np.repeat(ah, len(op)), np.repeat(ad, len(op)), np.tile(op, n)
        rec_in = (rflags[cls[o]][:, recs[0]] & flag) != 0 if recs else np.zeros(n, bool)
        if recs:
            cols, rows = m.rec_shape[recs[0]]

        def path_a():
            return m.snapshot_objects_obj(o, views, stats=st)

        def path_b():
            vals = np.zeros((n, K), np.uint64)
            heads = np.zeros((n, K), np.uint64)
            keep = np.zeros((n, K), bool)
            if len(ip):
                v = m.get_props(bh_i, bd_i, bp_i).reshape(n, len(ip))
                vals[:, :len(ip)] = v
                ki = ip < n_int
                keep[:, :len(ip)][:, ki] = v[:, ki] != 0
                f = v[:, ~ki].view(np.float64)
                with np.errstate(invalid="ignore"):
                    keep[:, :len(ip)][:, ~ki] = (f > 0.001) | (f < -0.001)
            if len(op):
                vh, vd = m.get_objects(bh_o, bd_o, bp_o)
                vals[:, len(ip):] = vd.view(np.uint64).reshape(n, len(op))
                heads[:, len(ip):] = vh.view(np.uint64).reshape(n, len(op))
                keep[:, len(ip):] = (vals[:, len(ip):] != 0) | (heads[:, len(ip):] != 0)
            keep &= in_view
            out = {"p_count": keep.sum(1).astype(np.uint32), "p_pid": np.broadcast_to(pids, (n, K))[keep],
                   "p_bits": vals[keep], "p_head": heads[keep]}
            if recs:
                who = np.nonzero(rec_in)[0]
                used = np.zeros(len(who), np.uint64)
                m._chk(m.lib.nfk_get_used_rows(m.h, len(who), kernel._p(np.ascontiguousarray(ah[who])),
                                               kernel._p(np.ascontiguousarray(ad[who])),
                                               kernel._p(np.full(len(who), recs[0], np.int32)), kernel._p(used)))
                bit = ((used[:, None] >> np.arange(rows, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
                bit3 = np.broadcast_to(bit[:, None, :], (len(who), cols, rows))   # entry-wise column-major
                e, c, r = np.nonzero(bit3)
                cells = m.get_records(ah[who][e], ad[who][e], np.full(len(e), recs[0], np.int32), r.astype(np.int32),
                                      c.astype(np.int32))
                out.update(r_count=rec_in.astype(np.uint32), r_used=used, cells=cells)
            return out

        ra, rb = path_a(), path_b()
        assert st["n_host"] == 0
        for k in ("p_count", "p_pid", "p_bits") + (("r_count", "r_used", "cells") if recs else ()):
            assert np.array_equal(ra[k], rb[k]), f"{name} n={n}: the two paths disagree in {k}"
        if ra["p_head"] is not None:
            assert np.array_equal(ra["p_head"], rb["p_head"]), f"{name} n={n}: the two paths disagree in p_head"
        n_words = int(in_view.sum()) + int(in_view[:, len(ip):].sum())
        n_ent, n_rent, n_cells = len(ra["p_pid"]), len(ra["r_rec"]), len(ra["cells"])
        nbytes = 8 * n + 8 * n_words + 20 * n_ent + 24 * n_rent + 16 * n_cells
        m.set_profiling(True)
        reps_a = 20 if n <= 4096 else (5 if n <= 65536 else 2)
        reps_b = 5 if n <= 4096 else 1
        ta, tb, ka = [], [], []
        for _ in range(rounds):
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
        gbps = nbytes / (np.median(ka) * 1e-3) / 1e9 if np.median(ka) > 0 else 0.0
        faster = max(ta) < min(tb)
        ok = ok and (faster or n < 4096)
        emit("n = %-7d (a) nfk_snapshot_objects_obj: wall %.3f (%.3f .. %.3f)  kernels %.4f  %d entries, %d record entries, "
             "%d cells, %d bytes -> %.0f GB/s (%.1f%% of the %d GB/s read-write mix)  read back %d bytes"
             % (n, np.median(ta), min(ta), max(ta), np.median(ka), n_ent, n_rent, n_cells, nbytes, gbps,
                100 * gbps / ceiling, ceiling, st["bytes"]))
        emit("            (b) get_props / get_objects / get_used_rows / get_records + numpy filter: wall %.3f (%.3f .. %.3f)   "
             "(b) / (a) = %.1f   %s"
             % (np.median(tb), min(tb), max(tb), np.median(tb) / np.median(ta),
                "(a) faster in every round" if faster else "(a) NOT faster beyond the rounds' spread"))
    m.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--n-obj", type=int, default=1 << 20)
    ap.add_argument("--n-rec-obj", type=int, default=500_000)
    ap.add_argument("--sizes", default="256,4096,65536,1048576")
    ap.add_argument("--rec-sizes", default="1,4096,500000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with open(os.path.join(ROOT, "profiles", "hbm_ceiling.json")) as f:
        ceiling = json.load(f)["kernels"]["copy_1_1"]["GBps"]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept as it grows: a long run leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    ok = True
    if a.sizes:
        w = workload.bench_world(n_obj=a.n_obj, groups=min(4096, max(a.n_obj // 256, 1)), n_ticks=4)
        ok = bench("config[1]'s world", w, kernel.VIEW_PUBLIC, a.sizes.split(","), a.rounds, ceiling, emit) and ok
    if a.rec_sizes:
        w = workload.record_world(n_ticks=4, n_obj=a.n_rec_obj, groups=max(a.n_rec_obj // 16, 1))
        ok = bench("config[4]'s world", w, kernel.VIEW_PRIVATE, a.rec_sizes.split(","), a.rounds, ceiling, emit) and ok
    emit("the LDS-staged variant of k_snap<true> (a wave's entries stored densely) was not built and not measured")
    assert ok, "nfk_snapshot_objects_obj is not faster than the get_props / get_records path at every n >= 4096"


if __name__ == "__main__":
    main()
