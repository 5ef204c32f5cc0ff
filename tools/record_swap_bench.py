"""Moving a record row on config[4]'s world shape (workload.record_world: players with a 64-row skill
record each): one window in which N objects each move one used row into an unused one,

  (a) by nfk_swap_rows: one batched call, one Swap event per object;
  (b) the only way without it: read the row (nfk_get_records of its cells), Remove it, AddRow(target,
      values) — a device read and two queued calls per object, Del + Add events.

Per window the call time (host clock around the batched calls, the read's stream synchronisation
included) and the frame time (host clock around nfk_execute + nfk_sync; the device time of the frame's
timer scopes from nfk_kernel_times: `aux` holds k_rs_scatter / k_rsets / k_rrows and the SetProperty
fold, `k_records` holds k_records and the two k_rset_slots passes).  The two ways alternate, --rounds
rounds after one warm-up round; every window moves other rows of the same objects, so each starts from
a comparable state.  Before anything is timed one window of each way is checked: the used masks and
the moved cells after the frame are what the move says.

usage: python tools/record_swap_bench.py [--n-obj 65536] [--n 4096] [--rounds 6] [--out profiles/record_swap.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noahgameframe_amd import kernel, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.record_world(n_ticks=2, n_obj=a.n_obj, groups=max(a.n_obj // 16, 1))
    # (the workload's own record calls stay out of the timed windows: only its first frames run)
    rows, cols = int(w["rec_rows"][0]), int(w["rec_cols"][0])
    gh, gd = w["guid_head"], w["guid_data"]
    m = kernel.world_from_workload(w)
    for t in range(2):
        kernel.run_workload(m, w, t, collect=False)
    m.synchronize()
    now = [int(w["tick_time"][1])]
    rng = np.random.default_rng(3)
    o = np.sort(rng.permutation(a.n_obj)[:a.n])
    ah, ad = np.ascontiguousarray(gh[o]), np.ascontiguousarray(gd[o])
    rec = np.zeros(a.n, np.int32)
    names = kernel.KERNEL_TIMER_NAMES

    def pick():
        """per object one used row and one unused row (objects without either keep out)"""
        um = m.get_used_rows(ah, ad, rec)
        bits = (um[:, None] >> np.arange(rows, dtype=np.uint64)[None, :]) & np.uint64(1)
        has = bits.any(1) & (bits == 0).any(1)
        k = rng.integers(0, rows, a.n)
        origin = np.array([np.nonzero(b)[0][kk % int(b.sum())] if h else 0 for b, kk, h in zip(bits, k, has)], np.int32)
        target = np.array([np.nonzero(b == 0)[0][kk % int((b == 0).sum())] if h else 0 for b, kk, h in zip(bits, k, has)],
                          np.int32)
        return has, origin, target, um

    def frame():
        now[0] += 100
        m.reset_kernel_times()
        t0 = time.perf_counter()
        m.Execute(now[0])
        m.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms, _, _ = m.kernel_times()
        return wall, {n: float(x) for n, x in zip(names, ms)}

    def by_swap(has, origin, target):
        t0 = time.perf_counter()
        m.swap_rows(ah[has], ad[has], rec[has], origin[has], target[has])
        return (time.perf_counter() - t0) * 1e3

    def by_remove_add(has, origin, target):
        n = int(has.sum())
        t0 = time.perf_counter()
        vals = np.zeros((n, 16), np.uint64)
        vals[:, :cols] = m.get_records(np.repeat(ah[has], cols), np.repeat(ad[has], cols), np.zeros(n * cols, np.int32),
                                       np.repeat(origin[has], cols), np.tile(np.arange(cols, dtype=np.int32), n)).reshape(n, cols)
        m.record_rows(ah[has], ad[has], rec[has], np.full(n, 2, np.int32), origin[has])
        m.record_rows(ah[has], ad[has], rec[has], np.full(n, 1, np.int32), target[has], vals)
        return (time.perf_counter() - t0) * 1e3

    def check(way):
        has, origin, target, um = pick()
        before = m.read_record(0)[o]
        way(has, origin, target)
        frame()
        after = m.read_record(0)[o]
        um2 = m.get_used_rows(ah, ad, rec)
        one = np.uint64(1)
        want = np.where(has, (um & ~(one << origin.astype(np.uint64))) | (one << target.astype(np.uint64)), um)
        # (the frame's record programs run on the moved rows too: compare the used masks, and the cells of
        # the columns no program writes)
        assert np.array_equal(um2, want), way.__name__
        idx = np.nonzero(has)[0]
        assert np.array_equal(after[idx, 0, target[idx]], before[idx, 0, origin[idx]]), way.__name__

    m.set_profiling(True)
    check(by_swap)
    check(by_remove_add)
    res = {"swap": [], "remove_add": []}
    for rnd in range(a.rounds + 1):
        for name, way in (("swap", by_swap), ("remove_add", by_remove_add)):
            has, origin, target, _ = pick()
            call = way(has, origin, target)
            wall, kt = frame()
            if rnd:     # (round 0 warms both ways up)
                res[name].append((call, wall, kt["aux"], kt["k_records"], int(has.sum())))
    m.set_profiling(False)
    lines = [f"Moving one record row per object, N = {a.n} objects of {a.n_obj} (config[4]'s world shape: one {rows}-row, "
             f"{cols}-column record each); {a.rounds} alternating rounds after one warm-up round; median (min .. max), ms.",
             "call: host clock around the batched calls (b's includes its device read); frame: host clock around",
             "nfk_execute + nfk_sync; aux / k_records: device time of the frame's timer scopes (aux holds k_rrows,",
             "k_records holds k_rset_slots)."]
    for name, label in (("swap", "(a) nfk_swap_rows                     "), ("remove_add", "(b) get_records + Remove + AddRow     ")):
        x = np.array([r[:4] for r in res[name]])
        f = lambda c: "%.3f (%.3f .. %.3f)" % (np.median(x[:, c]), x[:, c].min(), x[:, c].max())
        lines.append(f"{label} moves {res[name][0][4]}: call {f(0)}   frame {f(1)}   aux {f(2)}   k_records {f(3)}")
    sa, sb = np.array([r[:2] for r in res["swap"]]), np.array([r[:2] for r in res["remove_add"]])
    lines.append("(b) / (a), medians: call %.2f   frame %.2f   call + frame %.2f"
                 % (np.median(sb[:, 0]) / np.median(sa[:, 0]), np.median(sb[:, 1]) / np.median(sa[:, 1]),
                    np.median(sb.sum(1)) / np.median(sa.sum(1))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    m.close()


if __name__ == "__main__":
    main()
