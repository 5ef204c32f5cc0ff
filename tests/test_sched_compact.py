"""CPU: the 8-byte schedule word's encode / decode in a stand-alone host program under the address and
undefined-behaviour sanitizers (tests/cpp/sched_word.cpp), and — by the oracle alone — that the worlds
of tests/sched_compact_worlds.py reach the edges the GPU tests pin (tests/test_gpu_sched_compact.py)."""
import os
import subprocess

import numpy as np

from noahgameframe_amd.workload import KID
from tests import sched_compact_worlds as scw
from tests.parity import ROOT, run_oracle


def test_word_round_trips_at_every_field_bound():
    path = os.path.join(ROOT, "tests", "cpp", "_bin", "sched_word_san")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build_host_programs()
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "sched_word: ok" in r.stdout


def _fired(ref, t, kind, objs):
    """remain after frame t's fire of `kind`, per object of objs (None where it did not fire)"""
    sel = ref[f"fi_t{t}_kind"] == kind
    rem = dict(zip(ref[f"fi_t{t}_obj"][sel].tolist(), ref[f"fi_t{t}_rem"][sel].tolist()))
    return [rem.get(int(o)) for o in objs]


def test_remain_world_crosses_the_field():
    w, pick, j = scw.remain_world()
    ref = run_oracle(w)
    o = w["s_obj"][pick]
    assert len(o) > 50 and set(j.tolist()) == {0, 1, 2, 3}
    for t in range(1, int(w["cfg"][7])):   # one fire per frame from frame 1 on
        assert _fired(ref, t, KID["Move"], o) == (scw.REM_LO + j - t).tolist()
    assert (ref["final_s_remain"][KID["Move"], o] < scw.REM_LO).all()


def test_next_world_crosses_the_window():
    w, objs, r = scw.next_world()
    ref = run_oracle(w)
    top = scw.epoch_of(w) + (1 << scw.NEXT_BITS)
    k = KID["Poison"]
    assert len(objs) == 200
    assert all(x is None for x in _fired(ref, 3, k, objs))
    for t in (4, 5, 6, 7, 8):
        assert all(x is not None for x in _fired(ref, t, k, objs)), t
    # five fires: the first leaves next, four add the 500 ms step
    assert np.array_equal(ref["final_s_next"][k, objs], top - 700 + r + 4 * 500)
    assert ref["final_s_present"][k, objs].all()


def test_steps_world_mixes_steps_in_every_kind():
    w = scw.steps_world()
    common = scw.common_steps(w)
    assert common == {KID[n]: scw.step_ms(iv) for n, iv in scw.COMMON_INTERVALS.items()}
    for n in scw.ODD_INTERVALS:
        for calls in ("s", "h"):
            st = {scw.step_ms(iv) for iv in w[calls + "_interval"][(w[calls + "_kind"] == KID[n])
                                                                    & (w["h_op"] == 1 if calls == "h" else True)]}
            assert (common[KID[n]] in st and len(st) >= 3) if calls == "s" else len(st) >= 2, (n, calls)
    assert {1, 2, 3} <= set(w["h_op"].tolist())
    m = scw.membership_world()
    assert (m["born"] > 0).sum() > 100 and len(m["d_obj"]) > 100 and len(m["sw_obj"]) > 100
