"""The per-Set logs (nfk_watch_props / nfk_read_chain) of tests/arith_edges.py's float_props and int_edges
worlds, frame by frame, into an .npz, with each frame's coalesced events beside them (the worker of
tests/test_gpu_arith_edges.py::test_per_set_log_follows_the_predicates; run as a process of its own because
the library reads NFGPU_CHAIN_U once).  Watched: every float property, HP and SP.
Usage: arith_edges_chain.py OUT.npz SEED"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noahgameframe_amd import kernel, workload as wl  # noqa: E402
from tests import arith_edges  # noqa: E402

WATCH = [wl.PID[p] for p in wl.FLT_PROPS + ["HP", "SP"]]


def main(path, seed):
    z = {}
    for name in ("float_props", "int_edges"):
        w = arith_edges.BUILDERS[name](seed)
        m = kernel.world_from_workload(w)
        m.watch_props(WATCH)
        for t in range(int(w["cfg"][7])):
            r = kernel.run_workload(m, w, t)
            for k, v in m.read_chain().items():
                z[f"{name}_t{t}_{k}"] = v
            for k in ("ev_obj", "ev_pid", "ev_old", "ev_new"):
                z[f"{name}_t{t}_{k}"] = r[k]
        m.close()
    np.savez(path, **z)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
