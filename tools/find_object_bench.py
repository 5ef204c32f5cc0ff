"""FindObject timing on config[4]'s world (workload.record_world: 500k players, each with a 64-row skill
record) with an object (NFGUID) column added to the record (physical columns 3 and 4: each row holds
the NFGUID of another player): "which rows of this player's record hold this NFGUID" for n players at
once through nfk_find_objects (k_find_objects), beside the yardstick in the same run: nfk_find_rows
(k_find_rows, the code as it was) on the int cooldown column of the same record, which reads half the
cell bytes.

After 4 frames, for n = 1, 4096, 65 536 and 500 000.  Wall times are host clocks around the whole call
(each ends in a stream synchronisation); the device time is the HIP-event time around the launch
(nfk_find_stats).  --rounds alternating rounds of the two finds per n; a round's figure is the median of
its repetitions, the spread is the range of the rounds' figures.  Before anything is timed the object
find's answer is compared with the model (a numpy compare of both halves over the used rows: nothing
writes the object column in this world) and the int find's with nfk_get_records + numpy on up to 4096
of its finds.  Bytes: descriptors (40 / 32), used masks (8), used cells (16 / 8 per used row), results (8).

usage: python tools/find_object_bench.py [--rounds 4] [--out profiles/record_object_500k.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noahgameframe_amd import kernel, workload  # noqa: E402

OCOL = 3   # the data half's physical column; the head half is OCOL + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--n-obj", type=int, default=500_000)
    ap.add_argument("--sizes", default="1,4096,65536,500000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.record_world(n_ticks=4, n_obj=a.n_obj, groups=max(a.n_obj // 16, 1))
    n_obj, rows = a.n_obj, int(w["rec_rows"][0])
    gh, gd = w["guid_head"], w["guid_data"]
    rng = np.random.default_rng(1)
    # the object column: every row names another player (a small pool per object, so a find hits several rows)
    pool = rng.integers(0, n_obj, (n_obj, 4))
    who = np.take_along_axis(pool, rng.integers(0, 4, (n_obj, rows)), 1)
    cells = np.zeros((n_obj, OCOL + 2, rows), np.uint64)
    cells[:, :OCOL] = w["rec0_cells"]
    cells[:, OCOL] = gd[who].view(np.uint64)
    cells[:, OCOL + 1] = gh[who].view(np.uint64)
    w["rec0_cells"] = cells
    w["rec_cols"] = np.array([OCOL + 2], np.int32)
    ct = w["rec_ctype"].copy()
    ct[0, OCOL], ct[0, OCOL + 1] = kernel.REC_OBJ_DATA, kernel.REC_OBJ_HEAD
    w["rec_ctype"] = ct
    m = kernel.world_from_workload(w)
    for t in range(4):
        kernel.run_workload(m, w, t, collect=False)
    m.synchronize()
    order = rng.permutation(n_obj)
    used_all = np.zeros(n_obj, np.uint64)
    m._chk(m.lib.nfk_get_used_rows(m.h, n_obj, kernel._p(gh), kernel._p(gd), kernel._p(np.zeros(n_obj, np.int32)),
                                   kernel._p(used_all)))
    weights = np.uint64(1) << np.arange(rows, dtype=np.uint64)
    st = {}
    nused = int(np.mean([bin(int(x)).count("1") for x in used_all[:4096]]))
    lines = [f"FindObject on config[4]'s world with an object column: {n_obj} objects, one {rows}-row record each "
             f"({nused} rows used on average); {a.rounds} alternating rounds, a round = the median of its repetitions; "
             "median (min .. max of the rounds), ms"]
    for n in [min(int(x), n_obj) for x in a.sizes.split(",")]:
        o = np.sort(order[:n])
        ah, ad = np.ascontiguousarray(gh[o]), np.ascontiguousarray(gd[o])
        rec = np.zeros(n, np.int32)
        ocol, icol = np.full(n, OCOL, np.int32), np.full(n, 1, np.int32)
        arg = pool[o, 0]                       # one of the object's pool: held by about a quarter of its rows
        vh, vd = np.ascontiguousarray(gh[arg]), np.ascontiguousarray(gd[arg])
        zero = np.zeros(n, np.uint64)

        def find_o():
            return m.find_objects(ah, ad, rec, ocol, vh, vd, stats=st)

        def find_i():
            return m.find_rows(ah, ad, rec, icol, zero, stats=st)

        # the model, before anything is timed
        eq = (cells[o, OCOL] == vd.view(np.uint64)[:, None]) & (cells[o, OCOL + 1] == vh.view(np.uint64)[:, None])
        want_o = (eq.astype(np.uint64) @ weights) & used_all[o]
        got_o = find_o()
        assert st["n_host"] == 0 and np.array_equal(got_o, want_o), f"n={n}: nfk_find_objects differs from the model"
        k = min(n, 4096)
        got_i = find_i()
        back = m.get_records(np.repeat(ah[:k], rows), np.repeat(ad[:k], rows), np.zeros(k * rows, np.int32),
                             np.tile(np.arange(rows, dtype=np.int32), k), np.full(k * rows, 1, np.int32)).reshape(k, rows)
        want_i = ((back == 0).astype(np.uint64) @ weights) & used_all[o[:k]]
        assert np.array_equal(got_i[:k], want_i), f"n={n}: nfk_find_rows differs from nfk_get_records"
        hits = int(sum(bin(int(x)).count("1") for x in got_o[:4096]))
        m.set_profiling(True)
        reps = 20 if n <= 4096 else (5 if n <= 65536 else 2)
        to, ti, ko, ki = [], [], [], []
        for _ in range(a.rounds):
            for f, tw, tk in ((find_o, to, ko), (find_i, ti, ki)):
                xs, ks = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    f()
                    xs.append((time.perf_counter() - t0) * 1e3)
                    ks.append(st["kernel_ms"])
                tw.append(float(np.median(xs)))
                tk.append(float(np.median(ks)))
        m.set_profiling(False)
        nu = int(sum(bin(int(x)).count("1") for x in used_all[o]))
        bo, bi = 56 * n + 16 * nu, 48 * n + 8 * nu
        lines.append("n = %-7d nfk_find_objects: wall %.3f (%.3f .. %.3f)  launch %.4f (%.4f .. %.4f)  %d bytes -> %.0f GB/s   hits in the first %d finds: %d"
                     % (n, np.median(to), min(to), max(to), np.median(ko), min(ko), max(ko), bo,
                        bo / (np.median(ko) * 1e-3) / 1e9 if np.median(ko) > 0 else 0.0, min(n, 4096), hits))
        lines.append("            nfk_find_rows (int): wall %.3f (%.3f .. %.3f)  launch %.4f (%.4f .. %.4f)  %d bytes -> %.0f GB/s   object / int: wall %.2f  launch %.2f"
                     % (np.median(ti), min(ti), max(ti), np.median(ki), min(ki), max(ki), bi,
                        bi / (np.median(ki) * 1e-3) / 1e9 if np.median(ki) > 0 else 0.0, np.median(to) / np.median(ti),
                        np.median(ko) / np.median(ki) if np.median(ki) > 0 else 0.0))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    m.close()


if __name__ == "__main__":
    main()
