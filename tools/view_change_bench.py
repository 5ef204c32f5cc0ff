"""Who must be told that an object entered or left, on config[2]'s world shape (workload.bench_world at
--n-obj objects): per window N players switch group inside their scene, and the lists
NFCSceneAOIModule::OnGroupEvent reads inside each SwitchScene (the old group's and the new group's
players and other objects, as of that call) are fetched

  (a) by one nfk_view_changes call after the window's N nfk_switch_scene calls;
  (b) the only exact way before it, on the same library: one nfk_query_objects batch per switch (old
      and new group, players and others, the mover left out), issued before that switch is queued.

Per window the time of the list calls alone (host clock; the N nfk_switch_scene calls, the same in both
ways, are timed apart) and (a)'s kernel_ms.  The two ways alternate on two worlds, --rounds rounds after
one warm-up round; the lists of the two ways are compared in the warm-up round.

usage: python tools/view_change_bench.py [--n-obj 65536] [--n 4096] [--rounds 6] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noahgameframe_amd import kernel, workload  # noqa: E402
from noahgameframe_amd.kernel import Q_OTHERS, Q_PLAYERS, query  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = max(a.n_obj // 256, 2)
    w = workload.bench_world(n_obj=a.n_obj, groups=groups, players_per_group=32, n_ticks=a.rounds + 2)
    gh, gd = w["guid_head"], w["guid_data"]
    worlds = {k: kernel.world_from_workload(w, capacity=a.n_obj + a.n_obj // 8, slack_per_256=8) for k in ("view", "query")}
    for m in worlds.values():
        m.set_profiling(True)
    scene = np.array(w["scene"], np.int32)
    group = np.array(w["group"], np.int32)
    players = np.nonzero(w["is_player"])[0]
    assert len(players) >= a.n
    rng = np.random.default_rng(9)
    res = {"view": [], "query": []}
    for rnd in range(a.rounds + 1):
        movers = rng.permutation(players)[:a.n]
        to = (group[movers] % groups + 1).astype(np.int32)   # the next group of the scene
        lists = {}
        for name, m in worlds.items():
            t_list = t_sw = 0.0
            got = []
            for o, g1 in zip(movers.tolist(), to.tolist()):
                if name == "query":
                    s, g0 = int(scene[o]), int(group[o])
                    t0 = time.perf_counter()
                    got += m.query_objects([query(s, g0, Q_PLAYERS, skip_obj=o), query(s, g0, Q_OTHERS, skip_obj=o),
                                            query(s, g1, Q_PLAYERS, skip_obj=o), query(s, g1, Q_OTHERS, skip_obj=o)])
                    t_list += time.perf_counter() - t0
                t0 = time.perf_counter()
                m.SwitchScene((int(gh[o]), int(gd[o])), int(scene[o]), g1, 0.0, 0.0, 0.0)
                t_sw += time.perf_counter() - t0
            kms = 0.0
            if name == "view":
                t0 = time.perf_counter()
                vc = m.view_changes()
                t_list = time.perf_counter() - t0
                kms = vc["kernel_ms"]
                assert vc["n_host"] == 0
                off, obj = vc["visit_off"], vc["obj"]
                got = [obj[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
            lists[name] = got
            m.Execute(int(w["tick_time"][rnd]))
            m.synchronize()
            if rnd:     # (round 0 warms both ways up)
                res[name].append((t_list * 1e3, t_sw * 1e3, kms))
        if rnd == 0:    # (a switch within a scene between groups > 0: two visits, four lists, as way (b) asks)
            assert len(lists["view"]) == len(lists["query"]) == 4 * a.n
            for x, y in zip(lists["view"], lists["query"]):
                assert np.array_equal(x, y)
        group[movers] = to
    lines = [f"N = {a.n} players of {a.n_obj} objects ({groups} groups, 32 players each: config[2]'s world shape) switch group per "
             f"window; {a.rounds} alternating rounds after one warm-up round; median (min .. max), ms.",
             "lists: host clock around the list calls of one window; switches: around its N nfk_switch_scene calls (Python,",
             "one ctypes call each); kernel: nfk_view_changes' kernel_ms.  Both ways on this change's library; their lists are",
             "equal in the warm-up round."]
    for name, label in (("view", "(a) one nfk_view_changes per window        "),
                        ("query", "(b) one nfk_query_objects batch per switch ")):
        x = np.array(res[name])
        f = lambda c: "%.3f (%.3f .. %.3f)" % (np.median(x[:, c]), x[:, c].min(), x[:, c].max())
        lines.append(f"{label} lists {f(0)}   switches {f(1)}" + (f"   kernel {f(2)}" if name == "view" else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    for m in worlds.values():
        m.close()


if __name__ == "__main__":
    main()
