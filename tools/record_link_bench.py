"""A level-up on config[4]'s world shape (workload.record_world: players with a 64-row skill record
each) with the reference's CommPropertyValue record beside it (7 rows x 16 int columns, every row
used): per window N objects take a level-up, 16 SetRecordInt calls on row 0 (RefreshBaseProperty), and
the 14 int properties no heartbeat program writes follow their columns' sums,

  (a) by the link (nfk_link_record): the Sets are queued, the device sums in the frame;
  (b) the only way without it, on the same library in a world without the link: the Sets are queued,
      then nfk_get_records of the 7 rows of every linked column (read-your-writes), a host sum (int32
      cells, a 32-bit add) and nfk_set_props of the sums.

Per window the call time (host clock around the batched calls; b's includes its device reads) and
the frame time (host clock around nfk_execute + nfk_sync), and the device time of the frame's `aux`
timer scope, which holds k_rsets / k_rrows / k_links and the SetProperty fold (k_sets); k_rrows and
k_links are not timed apart from it.  The two ways alternate, --rounds rounds after one warm-up round.
Before anything is timed, and after the last round, the linked properties of the two worlds are
compared: equal in every object.

usage: python tools/record_link_bench.py [--n-obj 65536] [--n 4096] [--rounds 6] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noahgameframe_amd import kernel, workload  # noqa: E402

ROWS, COLS = 7, 16
# the int properties no program of the workload writes, one per column; two columns have no link
LINKED = [workload.PID[n] for n in ("MAXHP", "HPREGEN", "MAXMP", "MPREGEN", "SP", "MAXSP", "SPREGEN", "EXP", "Gold",
                                    "Level", "ATK_VALUE", "DEF_VALUE", "Camp", "NPCType")]
COL_PID = LINKED + [-1, -1]


def build(w, link, cells):
    """kernel.world_from_workload with one more record, the linked one"""
    n_obj, n_int, n_flt, n_cls, n_kind, n_rec = (int(x) for x in w["cfg"][:6])
    m = kernel.NFKernelModule(n_obj, n_int, n_flt, n_cls, n_kind, n_rec + 1)
    for c in range(n_cls):
        m.set_prop_flags(c, w["prop_flags"][c])
    for r in range(n_rec):
        m.define_record(r, int(w["rec_rows"][r]), int(w["rec_cols"][r]), w["rec_ctype"][r], w["rec_flags"][:, r])
    m.define_record(n_rec, ROWS, COLS, [0] * COLS, [workload.PRIVATE] * n_cls)
    for k in range(n_kind):
        m.define_kind(k, w["ops"][k][: int(w["n_ops"][k])])
    if link:
        m.link_record(n_rec, ROWS, COL_PID)
    m.create_objects(w["guid_head"], w["guid_data"], w["scene"], w["group"], w["cls"], w["is_player"])
    for p in range(n_int):
        m.load_prop(p, w["init_i"][p])
    for p in range(n_flt):
        m.load_prop(n_int + p, w["init_f"][p])
    for r in range(n_rec):
        m.load_record(r, w[f"rec{r}_cells"], w[f"rec{r}_used"])
    m.load_record(n_rec, cells, np.full(n_obj, (1 << ROWS) - 1, np.uint64))
    m.commit()
    so = w["s_obj"]
    m.add_schedules(w["guid_head"][so], w["guid_data"][so], w["s_kind"], w["s_interval"], w["s_count"], w["s_time"])
    return m, n_rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = workload.record_world(n_ticks=2, n_obj=a.n_obj, groups=max(a.n_obj // 16, 1))
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 100, (a.n_obj, COLS, ROWS)).astype(np.uint64)
    gh, gd = w["guid_head"], w["guid_data"]
    worlds = {}
    for name, link in (("link", True), ("host", False)):
        m, rec = build(w, link, cells)
        m.set_profiling(True)
        worlds[name] = m
    now = [int(w["tick_time"][0])]
    names = kernel.KERNEL_TIMER_NAMES
    lcols = np.array([c for c in range(COLS) if COL_PID[c] >= 0], np.int32)
    lpids = np.array([COL_PID[c] for c in lcols], np.int32)

    def frame(m):
        m.reset_kernel_times()
        t0 = time.perf_counter()
        m.Execute(now[0])
        m.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms, _, _ = m.kernel_times()
        return wall, {n: float(x) for n, x in zip(names, ms)}

    def level_up(m, o, vals):
        """16 Sets on row 0 of each object, one batched call"""
        n = len(o)
        m.set_records(np.repeat(gh[o], COLS), np.repeat(gd[o], COLS), np.full(n * COLS, rec, np.int32),
                      np.zeros(n * COLS, np.int32), np.tile(np.arange(COLS, dtype=np.int32), n), vals.reshape(-1))

    def by_link(o, vals):
        t0 = time.perf_counter()
        level_up(worlds["link"], o, vals)
        return (time.perf_counter() - t0) * 1e3

    def by_host(o, vals):
        m, n, k = worlds["host"], len(o), len(lcols)
        t0 = time.perf_counter()
        level_up(m, o, vals)
        # the 7 rows of every linked column of every object: [n][k][ROWS]
        qo = np.repeat(o, k * ROWS)
        got = m.get_records(gh[qo], gd[qo], np.full(n * k * ROWS, rec, np.int32),
                            np.tile(np.arange(ROWS, dtype=np.int32), n * k), np.tile(np.repeat(lcols, ROWS), n))
        sums = got.astype(np.uint32).reshape(n, k, ROWS).sum(2, dtype=np.uint32).astype(np.int32).astype(np.int64)
        po = np.repeat(o, k)
        m.set_props(gh[po], gd[po], np.tile(lpids, n), sums.reshape(-1).view(np.uint64))
        return (time.perf_counter() - t0) * 1e3

    def same(tag):
        for p in LINKED:
            x, y = worlds["link"].read_prop(p), worlds["host"].read_prop(p)
            assert np.array_equal(x, y), (tag, p)

    res = {"link": [], "host": []}
    n_ev = {}
    for rnd in range(a.rounds + 1):
        o = np.sort(rng.permutation(a.n_obj)[:a.n])
        # (values no cell holds yet, so that every Set is accepted: an unchanged Set raises no event and
        # the reference leaves the property alone, where way (b) would still write its sum)
        vals = (1000 * (rnd + 1) + rng.integers(0, 1000, (a.n, COLS))).astype(np.uint64)
        now[0] += 100
        for name, way in (("link", by_link), ("host", by_host)):
            call = way(o, vals)
            wall, kt = frame(worlds[name])
            n_ev[name] = worlds[name].summary()["n_prop_events"]
            if rnd:     # (round 0 warms both ways up)
                res[name].append((call, wall, kt["aux"]))
        assert n_ev["link"] == n_ev["host"], n_ev
        if rnd in (0, a.rounds):
            same(f"round {rnd}")
    lines = [f"A level-up of N = {a.n} objects of {a.n_obj} per window (config[4]'s world shape plus a {ROWS} x {COLS} linked record, "
             f"{len(lpids)} linked columns): 16 Sets on row 0 per object; {a.rounds} alternating rounds after one warm-up round; "
             "median (min .. max), ms.",
             "call: host clock around the batched calls (b's includes its device reads); frame: host clock around nfk_execute +",
             "nfk_sync; aux: device time of the frame's timer scope that holds k_rsets / k_rrows / k_links and the SetProperty fold",
             "(k_rrows and k_links were not timed apart from it).  Both ways on this change's library; the linked properties of",
             "the two worlds are equal in every object before and after the timed rounds."]
    for name, label in (("link", "(a) nfk_link_record                          "),
                        ("host", "(b) get_records + host sums + nfk_set_props  ")):
        x = np.array(res[name])
        f = lambda c: "%.3f (%.3f .. %.3f)" % (np.median(x[:, c]), x[:, c].min(), x[:, c].max())
        lines.append(f"{label} call {f(0)}   frame {f(1)}   aux {f(2)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    for m in worlds.values():
        m.close()


if __name__ == "__main__":
    main()
