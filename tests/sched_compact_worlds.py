"""Worlds at the edges of the 8-byte schedule word (csrc/nfgpu_device.hpp: flags, next as a 33-bit
offset from the world's epoch, a 27-bit signed remain, the step one common value per kind), shared by
tests/test_sched_compact.py (CPU: the oracle alone shows each world reaches its edge) and
tests/test_gpu_sched_compact.py (GPU: every kernel path against the oracle and an all-wide twin).

The constants restate the header's; the GPU tests fail on the forms read-back if they drift."""
import numpy as np

from noahgameframe_amd import workload
from noahgameframe_amd.workload import KID

NEXT_BITS, REM_BITS, EPOCH_BACK = 33, 27, 1 << 30
REM_LO = -(1 << (REM_BITS - 1))            # the lowest remain a word holds
SMALL = dict(n_obj=3000, n_scenes=2, groups_per_scene=6, players_per_group=3)


def step_ms(interval):
    """(int64)(interval * 1000.0f) as the schedule module computes it (SM:71)"""
    return int(np.float32(interval) * np.float32(1000.0))


def epoch_of(w):
    """the epoch the device fixes: the world's first AddSchedule call's time less EPOCH_BACK"""
    return int(w["s_time"][0]) - EPOCH_BACK


def remain_world(n_ticks=10, seed=5):
    """Forever Move heartbeats (0.1 s, the kind's common step, one fire per 100 ms frame from frame
    1 on) whose count is REM_LO + j, j in 0..3: remain after frame t is REM_LO + j - t, which leaves
    the word's field in frame j + 1.  Returns (world, picked schedule indices, their j)."""
    w = workload.make_world(n_ticks=n_ticks, seed=seed, host_ops=False, **SMALL)
    rng = np.random.default_rng(seed)
    move = np.nonzero(w["s_kind"] == KID["Move"])[0]
    pick = move[rng.random(len(move)) < 0.1]
    j = rng.integers(0, 4, len(pick))
    w["s_count"][pick] = (REM_LO + j).astype(np.int32)
    return w, pick, j


def next_world(n_ticks=9, seed=6):
    """Poison schedules (0.5 s, the kind's common step; counted and forever) added in window 3 with a
    start time such that next = top - 700 + r (top: the first time past the epoch window, r in 0..3),
    and frame times that jump to the top of the window: frames 4 and 5 fire them inside the window
    (the first fire leaves next, the second adds the step: top - 200 + r), frame 6 carries next over
    the top (top + 300 + r), frames 7 and 8 fire the wide record.  Returns (world, objects, r)."""
    w = workload.make_world(n_ticks=n_ticks, seed=seed, host_ops=False, **SMALL)
    rng = np.random.default_rng(seed)
    top = epoch_of(w) + (1 << NEXT_BITS)
    n_obj = int(w["cfg"][0])
    has = np.zeros(n_obj, bool)
    has[w["s_obj"][w["s_kind"] == KID["Poison"]]] = True
    objs = np.nonzero(~has)[0][:200]
    r = rng.integers(0, 4, len(objs))
    tt = w["tick_time"].copy()
    tt[3:] = top + np.array([-1200, -600, -500, 0, 600, 1200])[: n_ticks - 3]
    w["tick_time"] = tt
    m = len(objs)
    w["h_tick"] = np.full(m, 3, np.int32)
    w["h_op"] = np.ones(m, np.int32)
    w["h_obj"] = objs.astype(np.int32)
    w["h_kind"] = np.full(m, KID["Poison"], np.int32)
    w["h_interval"] = np.full(m, 0.5, np.float32)
    w["h_count"] = np.where(np.arange(m) % 2 == 0, -1, 6).astype(np.int32)
    w["h_time"] = (top - 1200 + r).astype(np.int64)
    return w, objs, r


# steps beside a kind's common one: 1 ms off either way, the opposite sign, and the sched_edges ones
COMMON_INTERVALS = {"HPRegen": 1.0, "MPRegen": 2.0, "Move": 0.1, "Patrol": 3.0, "Poison": 0.5}   # (workload.make_world's spec)
ODD_INTERVALS = {"HPRegen": [1.0015, 0.9985, -1.0], "MPRegen": [2.0015, -2.0], "Move": [0.1015, -0.1],
                 "Poison": [0.5015, 0.4985, -0.5]}


def steps_world(n_ticks=10, seed=7, **kw):
    """sched_edges' schedules (steps beyond 28 bits, negative, 0.05 s beside the kind's 1 s, remain
    wrapping through INT32_MIN, zero counts) plus, at commit and through schedule calls in every
    window, schedules whose step is 1 ms off their kind's common step or its negative; the generator's
    own schedule calls (host_ops) remove by name, remove all and re-add on the same objects."""
    opts = dict(SMALL, sched_edges=True, host_ops=True)
    opts.update(kw)
    w = workload.make_world(n_ticks=n_ticks, seed=seed, **opts)
    rng = np.random.default_rng(seed)
    for name, ivs in ODD_INTERVALS.items():
        assert all(step_ms(iv) != step_ms(COMMON_INTERVALS[name]) for iv in ivs), name
        idx = np.nonzero(w["s_kind"] == KID[name])[0]
        idx = idx[1:][rng.random(len(idx) - 1) < 0.04]     # (never the world's first call: it fixes the epoch)
        w["s_interval"][idx] = rng.choice(np.array(ivs, np.float32), len(idx))
    # schedule calls with odd steps: appended to each window's calls, on objects of any state
    n_obj = int(w["cfg"][0])
    born = w.get("born")
    extra = {k: [] for k in ("h_tick", "h_op", "h_obj", "h_kind", "h_interval", "h_count", "h_time")}
    for t in range(1, n_ticks):
        m = 40
        o = rng.integers(0, n_obj, m)
        if born is not None:   # (calls on live objects only: see workload._lifecycle_world)
            died = np.full(n_obj, 1 << 30)
            died[w["d_obj"]] = w["d_tick"]
            o = o[(born[o] < t) & (died[o] > t)]
            m = len(o)
        names = rng.choice(list(ODD_INTERVALS), m)
        extra["h_tick"].append(np.full(m, t))
        extra["h_op"].append(np.ones(m))
        extra["h_obj"].append(o)
        extra["h_kind"].append(np.array([KID[n] for n in names]))
        extra["h_interval"].append(np.array([rng.choice(ODD_INTERVALS[n]) for n in names]))
        extra["h_count"].append(np.where(rng.random(m) < 0.5, -1, rng.integers(1, 5, m)))
        extra["h_time"].append(int(w["tick_time"][t - 1]) + rng.integers(0, 100, m))
    merged = {k: np.concatenate([w[k]] + extra[k]).astype(w[k].dtype) for k in extra}
    order = np.argsort(merged["h_tick"], kind="stable")     # a window's own calls first, then the odd ones
    for k in merged:
        w[k] = merged[k][order]
    return w


def membership_world(n_ticks=10, seed=8):
    """steps_world with SwitchScene (new groups too), CreateObject and DestroyObject between frames:
    rows carry both forms between slots, and destroyed objects' slots are reused or left slack."""
    return steps_world(n_ticks, seed, n_scenes=3, switch_frac=0.03, switch_new_groups=True, spawn_frac=0.03,
                       destroy_frac=0.03)


def common_steps(w):
    """per kind: the most frequent step among the AddSchedule calls made before frame 0"""
    out = {}
    for k in np.unique(w["s_kind"]):
        st = [step_ms(iv) for iv in w["s_interval"][w["s_kind"] == k]]
        vals, cnt = np.unique(st, return_counts=True)
        out[int(k)] = int(vals[np.argmax(cnt)])
    return out
