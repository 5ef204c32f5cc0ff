"""CPU: the heavy-churn worlds of tests/churn_worlds.py reach the membership edges they are made for
(conditions on the workload alone), the oracle equals the compiled reference over their long runs, the
`churn` golden is the world its generator names, and GuidMap with its mirror log holds against a std::map
(tests/cpp/guidmap_churn.cpp, plain and under the host sanitizers)."""
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import nfio, workload
from tests import churn_worlds as cw
from tests.parity import REF, ROOT, compare_runs, run_oracle, run_ref
from tests.test_oracle import SESSION, _compare_dirty_sync

GOLDEN = os.path.join(ROOT, "tests", "golden")
have_ref = os.path.exists(REF)
# the arrivals' row buffer's first size and the per-object reserve made at commit (nfgpu_host.hip)
ARRIVAL_ROWS = 1024
reserve = lambda n0: n0 + n0 // 4 + 4096


def _born(w):
    return np.asarray(w["born"]) if "born" in w else np.full(len(w["guid_head"]), -1, np.int32)


def _windows_with(w, spawn=True):
    born, n = _born(w), 0
    for t in range(int(w["cfg"][7])):
        sw = np.any((w["sw_tick"] == t) & (w["sw_scene"] >= 0))
        n += bool((np.any(born == t) or not spawn) and np.any(w["d_tick"] == t) and sw)
    return n


def test_tiny_groups_drains_and_refills():
    ms = cw.membership(cw.world("tiny_groups"))
    drained = ms.drained()
    assert len(drained) >= 4, [ms.pairs[p] for p in drained]
    assert all(ms.refilled_at(p) for p in drained)
    # the objects that join a pair somebody left before are most of the world by the end
    assert ms.reused[-1].sum() > ms.alive[-1].sum() // 2


def test_grow_passes_the_reserve_and_the_table_doublings():
    w = cw.world("grow")
    n0 = int(np.sum(_born(w) < 0))
    assert len(w["guid_head"]) > reserve(n0), (len(w["guid_head"]), reserve(n0))
    live = cw.membership(w).alive.sum(1)
    assert live[0] < 512 and np.any(live > 512) and np.any(live > 1024), (live[0], live.max())


def test_burst_outgrows_the_arrival_rows():
    w = cw.world("burst")
    per_window = np.bincount(_born(w)[_born(w) >= 0])
    assert per_window.max() > ARRIVAL_ROWS, per_window.max()
    assert int(w["cfg"][5]) == 1   # records: wide rows


def test_drain_empties():
    w = cw.world("drain")
    assert not np.any(_born(w) >= 0) and "d_tick" in w   # destroy-only
    ms = cw.membership(w)
    assert np.any(ms.counts[-1] == 0)
    assert ms.alive[-1].sum() * 10 < len(w["guid_head"]), ms.alive[-1].sum()
    assert int(w["n_oprops"][0]) == len(workload.OBJ_PROPS)


@pytest.mark.parametrize("name", sorted(cw.WORLDS))
def test_windows_hold_every_membership_call(name):
    """at least 10 windows with a spawn, a destroy and a SwitchScene to another cell together (drain is
    destroy-only: a destroy and a switch)"""
    w = cw.world(name)
    assert _windows_with(w, spawn=name != "drain") >= 10


def test_relayout_paths_by_the_layout_rule():
    """churn_worlds.relayouts — the layout's rule on the workload alone; tests/test_gpu_churn.py holds the
    device's membership_stats() to it — says which worlds reach both re-layout paths: with no slack every
    window is a full layout; tiny_groups and churn at slack 1 and 64 have full and segment windows.  At slack
    1 a segment has 2 free slots after a layout, so churn's one segment window is all its 8 segments allow
    (with 4 groups a scene, 14 segments, it had none at any seed from 1 to 119)"""
    for name in cw.WORLDS:
        n_full, n_seg = cw.relayouts(cw.world(name), -1)
        assert n_full >= 10 and n_seg == 0, (name, n_full, n_seg)
    for name, slack in (("tiny_groups", 1), ("tiny_groups", 64), ("churn", 1), ("churn", 64)):
        n_full, n_seg = cw.relayouts(cw.world(name), slack)
        assert n_full > 0 and n_seg > 0, (name, slack, n_full, n_seg)
    assert cw.relayouts(cw.world("churn"), 1) == (78, 1)
    assert cw.relayouts(cw.world("burst"), 64) == (0, 11)   # ample slack takes 1200 arrivals a window in place


def test_membership_helper_agrees_with_the_oracle():
    """the helper's final cells are the oracle's final SceneID / GroupID of every live object"""
    for name in ("tiny_groups", "drain"):
        w = cw.world(name)
        ms, o = cw.membership(w), run_oracle(w)
        live = np.nonzero(ms.alive[-1])[0]
        pairs = np.array(ms.pairs, np.int64)[ms.pair_of[-1][live]]
        assert np.array_equal(o["final_i"][workload.PID["SceneID"]][live], pairs[:, 0])
        assert np.array_equal(o["final_i"][workload.PID["GroupID"]][live], pairs[:, 1])


@pytest.mark.skipif(not have_ref, reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("name", ["churn", "grow", "tiny_groups", "drain"])
def test_oracle_matches_reference_over_long_churn(name):
    """(churn: its first 48 windows — the reference takes 31 s over all 80, its scene groups holding
    hundreds of objects by then; the churn fractions are whole)"""
    w = cw.world(name)
    if name == "churn":
        w = cw.truncated(w, 48)
    compare_runs(run_oracle(w), run_ref(w))


@pytest.mark.skipif(not os.path.exists(SESSION), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_matches_reference_modules_per_frame_tiny_groups(tmp_path):
    """tiny_groups frame by frame against the reference's own server modules (nf_ref_session's per-frame
    mode, as test_oracle.py::test_oracle_matches_reference_modules_per_frame): events, ordered recipient
    lists, record events, fired heartbeats, through groups that drain and fill again"""
    w = cw.world("tiny_groups")
    nt = int(w["cfg"][7])
    wp, fp, pp = str(tmp_path / "w.nfio"), str(tmp_path / "f.nfio"), str(tmp_path / "p.nfio")
    nfio.write(wp, w)
    r = subprocess.run([SESSION, wp, str(nt), "0", fp, pp], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    fr = nfio.read(pp)
    fr.update({k: v for k, v in nfio.read(fp).items() if k.startswith("final_")})
    n_ev, n_msg = _compare_dirty_sync(fr, run_oracle(w), nt, 0)
    assert n_ev > 300 and n_msg > 300, (n_ev, n_msg)


def test_churn_golden_is_the_named_world():
    """tests/golden/churn.workload.nfio is churn_worlds' golden world (test_oracle.py compares the oracle
    with its expected file), and the fixture is no larger than the largest one before it"""
    w = cw.world(cw.GOLDEN_WORLD, cw.GOLDEN_TICKS)
    g = nfio.read(os.path.join(GOLDEN, "churn.workload.nfio"))
    assert sorted(g) == sorted(w)
    for k in w:
        a, b = np.ascontiguousarray(g[k]), np.ascontiguousarray(w[k])
        assert a.nbytes == b.nbytes and a.tobytes() == b.tobytes(), k   # (ops: records read back as bytes)
    assert len(cw.membership(w).drained()) >= 4
    size = lambda n: os.path.getsize(os.path.join(GOLDEN, n))
    assert size("churn.expected.nfio") <= size("arith.expected.nfio")


@pytest.mark.parametrize("exe", ["guidmap_churn", "guidmap_churn_san"], ids=["plain", "asan-ubsan"])
def test_guidmap_against_std_map(exe):
    """include/nfgpu_guidmap.hpp in a stand-alone host program: 300 000 random operations against a
    std::map, probe runs across the wrap, growth through 11 rehashes, the mirror after every batch"""
    path = os.path.join(ROOT, "tests", "cpp", "_bin", exe)
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build_host_programs()
    r = subprocess.run([path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "guidmap_churn ok: 300000 random operations" in r.stdout
