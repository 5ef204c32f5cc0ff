"""The per-Set logs of the `replay` cell-guard twins, frame by frame, into an .npz (the worker of
tests/test_gpu_cell_guards.py::test_cell_guard_chain_matches_mirror_twin; run as a process of its own because
the library reads NFGPU_CHAIN_U and NFGPU_CHAIN_NO_CLOSURE once).
Usage: cell_guard_chain.py OUT.npz N_TICKS SEED [PROPERTY ...]   (the watched properties; none given: the
destinations of every guarded op)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noahgameframe_amd import kernel, workload as wl  # noqa: E402


def chains(w, n_ticks, watch):
    gd = (w["ops"]["flags"] & wl.GUARD) != 0
    watched = [wl.PID[p] for p in watch] or sorted({int(d) for d in w["ops"]["dst"][gd]})
    m = kernel.world_from_workload(w)
    m.watch_props(watched)
    out = []
    for t in range(n_ticks):
        kernel.run_workload(m, w, t, collect=False)
        out.append(m.read_chain())
    m.close()
    return out


def main(path, n_ticks, seed, watch):
    z = {}
    for twin in ("A", "B"):
        w = wl.make_world(cell_guards=("replay", twin), n_ticks=n_ticks, seed=seed)
        for t, c in enumerate(chains(w, n_ticks, watch)):
            for k, v in c.items():
                z[f"{twin.lower()}_t{t}_{k}"] = v
    np.savez(path, **z)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:])
