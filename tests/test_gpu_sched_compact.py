"""GPU: the 8-byte schedule word at the edges of its fields (tests/sched_compact_worlds.py), on the three
kernel paths.  Every world runs twice — as it is, and with every record forced wide
(NFGPU_ABLATE=1<<15, kAblSchedWide) — and both runs must equal the oracle frame by frame (events,
fired lists with their remains, recipients, final state) and each other in nfk_read_schedules after
every frame; nfk_read_schedule_forms says which records were compact and which wide."""
import numpy as np
import pytest

from noahgameframe_amd import kernel, workload
from noahgameframe_amd.workload import KID
from tests import sched_compact_worlds as scw
from tests.parity import compare_runs, run_oracle

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize("path", ["k_tick", "k_tick_dyn", "k_tick_touch"])
WIDE = 1 << 15

_worlds = {}


def world(name):
    """(the builder's result, the oracle's run of its world), computed once"""
    if name not in _worlds:
        made = getattr(scw, name)()
        w = made[0] if isinstance(made, tuple) else made
        _worlds[name] = (made, run_oracle(w))
    return _worlds[name]


def run_frames(w, slack=0):
    """tests.parity.run_gpu, with the schedule table and the record forms read after every frame"""
    m = kernel.world_from_workload(w, slack_per_256=slack)
    out, sched, forms = {}, [], []
    for t in range(int(w["cfg"][7])):
        r = kernel.run_workload(m, w, t)
        for k in ("ev_obj", "ev_pid", "ev_old", "ev_new", "re_obj", "re_rrc", "re_old", "re_new",
                  "fi_obj", "fi_kind", "fi_rem"):
            pfx, nm = k.split("_", 1)
            out[f"{pfx}_t{t}_{nm}"] = r[k]
        out[f"mo_t{t}_off"] = r["mo_off"]
        out[f"mr_t{t}_obj"] = r["mr_obj"]
        sched.append(m.read_schedules())
        forms.append(m.read_schedule_forms())
    n_int, n_flt = int(w["cfg"][1]), int(w["cfg"][2])
    out["final_i"] = np.stack([m.read_prop(p) for p in range(n_int)])
    out["final_f"] = np.stack([m.read_prop(n_int + p) for p in range(n_flt)])
    nx, rm, st = sched[-1]
    out["final_s_next"], out["final_s_remain"], out["final_s_present"] = nx, rm, (st & 1).astype(np.uint8)
    m.close()
    return out, sched, forms


def both_forms(monkeypatch, path, w, ref, slack=0):
    """the world compact and forced wide, each against the oracle and against the other; returns the
    compact run's per-frame (next, remain, state) and forms"""
    runs = []
    for wide in (0, WIDE):
        monkeypatch.setenv("NFGPU_ABLATE", str((8 if path == "k_tick_touch" else 0) | wide))
        monkeypatch.setenv("NFGPU_JIT", "0" if path == "k_tick_dyn" else "1")
        runs.append(run_frames(w, slack))
        compare_runs(runs[-1][0], ref)
    (got, sched, forms), (got_w, sched_w, forms_w) = runs
    compare_runs(got, got_w)
    for t, (a, b) in enumerate(zip(sched, sched_w)):
        for x, y, nm in zip(a, b, ("next", "remain", "state")):
            assert np.array_equal(x, y), f"frame {t}: read_schedules {nm} differs between the compact and the wide world"
        present = (a[2] & 1).astype(bool)
        assert np.array_equal(forms_w[t].astype(bool), present), f"frame {t}: a forced-wide world holds a compact record"
        assert not (forms[t].astype(bool) & ~present).any(), f"frame {t}: a wide form without a schedule"
    return sched, forms


@PATHS
def test_forever_remain_leaves_the_field(gpu_available, monkeypatch, path):
    """remain = REM_LO + j - t after frame t: compact while it fits 27 bits, wide from frame j + 1 on"""
    (w, pick, j), ref = world("remain_world")
    sched, forms = both_forms(monkeypatch, path, w, ref)
    o = w["s_obj"][pick]
    for t in range(len(forms)):
        rem = sched[t][1][KID["Move"], o]
        assert np.array_equal(rem, scw.REM_LO + j - t), f"frame {t}"
        assert np.array_equal(forms[t][KID["Move"], o], (t > j).astype(np.uint8)), f"frame {t}"
    # and nothing else of the world went wide
    other = np.ones(forms[-1].shape, bool)
    other[KID["Move"], o] = False
    assert not forms[-1][other].any()


@PATHS
def test_next_leaves_the_epoch_window(gpu_available, monkeypatch, path):
    """next = top - 700 + r, then top - 200 + r (frames 4, 5: compact), then top + 300 + r (frame 6: wide)"""
    (w, objs, r), ref = world("next_world")
    sched, forms = both_forms(monkeypatch, path, w, ref)
    top = scw.epoch_of(w) + (1 << scw.NEXT_BITS)
    k = KID["Poison"]
    for t, nxt in ((3, top - 700 + r), (4, top - 700 + r), (5, top - 200 + r), (6, top + 300 + r), (7, top + 800 + r)):
        assert np.array_equal(sched[t][0][k, objs], nxt), f"frame {t}"
        assert (forms[t][k, objs] == (1 if t >= 6 else 0)).all(), f"frame {t}"
    assert (sched[8][2][k, objs] & 1).all()       # still scheduled, counted and forever alike


@PATHS
def test_steps_beside_the_common_step(gpu_available, monkeypatch, path):
    """a schedule is compact exactly when its step is its kind's most frequent one and its count fits"""
    w, ref = world("steps_world")
    sched, forms = both_forms(monkeypatch, path, w, ref)
    common = scw.common_steps(w)
    st = np.array([scw.step_ms(iv) for iv in w["s_interval"]])
    cnt = w["s_count"].astype(np.int64)
    exp_wide = (st != np.array([common[int(k)] for k in w["s_kind"]])) | (cnt < scw.REM_LO) | (cnt >= -scw.REM_LO)
    assert exp_wide.any() and not exp_wide.all()
    assert np.array_equal(forms[0][w["s_kind"], w["s_obj"]], exp_wide.astype(np.uint8))   # (frame 0 fires none of them)
    for t in range(len(forms)):   # both forms in every frame, schedule calls and removals included
        present = (sched[t][2] & 1).astype(bool)
        assert forms[t].any() and (present & ~forms[t].astype(bool)).any(), f"frame {t}"


@PATHS
@pytest.mark.parametrize("slack", [0, 32])
def test_rows_carry_both_forms(gpu_available, monkeypatch, path, slack):
    """SwitchScene, CreateObject, DestroyObject and slot reuse on a world of both forms"""
    w, ref = world("membership_world")
    sched, forms = both_forms(monkeypatch, path, w, ref, slack)
    present = (sched[-1][2] & 1).astype(bool)
    assert forms[-1].any() and (present & ~forms[-1].astype(bool)).any()


def test_bench_shape_has_no_wide_record(gpu_available):
    """config[1]'s world at small size: every schedule stays compact (the scan's fallback never runs)"""
    w = workload.bench_world(n_obj=8192, groups=32, n_ticks=10)
    m = kernel.world_from_workload(w)
    for t in range(10):
        kernel.run_workload(m, w, t, collect=False)
    st, wide = m.read_schedules()[2], m.read_schedule_forms()
    m.close()
    assert (st & 1).sum() > 4 * 8192 and not wide.any()
