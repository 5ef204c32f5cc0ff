"""Worlds whose membership churns hard for many windows (a helper module of tests/test_churn.py,
tests/test_gpu_churn.py and tests/golden/gen_churn_golden.py; no tests in it).

Membership is the part of a frame that keeps state across windows: the segment table and its slack, the
slots one object vacates and another takes later, scene groups that empty and fill again, the per-object
host vectors past the reserve made at commit, the arrivals' row buffer, the NFGUID table and its device
mirror.  The other suites run 8-10 windows at 1-3 % create / destroy / SwitchScene; these run up to 80
windows at 5-30 %.  Every world keeps rec_float_op / rec_set_float off, so the compiled reference
(oracle/_ref/nf_ref_harness) runs it too.

  churn        800 objects at the start in 2 scene groups (8 with the groups SwitchScene creates), 9 %
               created and 8 % destroyed a window (about 1430 alive at the end), 15 % switched, records
               with Sets and row calls, the rescheduling edge cases: 80 windows
  grow         300 objects growing to about 1250 alive (5970 created in all: past the per-object reserve
               of n0 + n0/4 + 4096 made at commit, and through the NFGUID table's doublings)
  tiny_groups  160 objects in 16 groups of about ten, a quarter switched every window: scene groups
               drain to nobody and are joined again later
  drain        destroy-only: 600 objects fall to under 10 %, with object (NFGUID) properties, so 16-byte
               columns move through pack / unpack while the segments empty
  burst        4000 objects, 30 % (1200) created and 30 % destroyed a window: more arrivals in one
               window than the arrivals' row buffer first holds (1024 rows), with records (wide rows)

membership(w) replays only a workload's membership calls in numpy."""
import numpy as np

from noahgameframe_amd import workload

WORLDS = {
    # (spawn_frac above destroy_frac: the live count climbs by 8 a window, past 1024 and 1280, so the
    # tile count changes over the run at every slack setting; at 0.08 / 0.08 it stays at 800 = 4 tiles)
    # (one group a scene at the start and the three a scene that SwitchScene creates: 8 segments, few enough
    # that relayouts() finds a window that fits the 2 free slots a segment has at slack 1; with the 14
    # segments of 4 groups a scene no seed from 1 to 119 has one)
    "churn": dict(n_obj=800, n_scenes=2, groups_per_scene=1, players_per_group=5, n_ticks=80, seed=7,
                  switch_frac=0.15, switch_new_groups=True, spawn_frac=0.09, destroy_frac=0.08, ext_frac=0.05,
                  host_ops=True, sched_edges=True, records=True, rec_rows=8, rec_set_frac=0.05, rec_row_frac=0.05),
    "grow": dict(n_obj=300, n_scenes=1, groups_per_scene=3, players_per_group=4, n_ticks=64, seed=8,
                 spawn_frac=0.30, destroy_frac=0.25, switch_frac=0.05, ext_frac=0.05, host_ops=True),
    "tiny_groups": dict(n_obj=160, n_scenes=2, groups_per_scene=8, players_per_group=2, n_ticks=64, seed=10,
                        spawn_frac=0.05, destroy_frac=0.05, switch_frac=0.25, switch_new_groups=True, ext_frac=0.1,
                        host_ops=True, records=True, rec_rows=8, rec_row_frac=0.1, rec_set_frac=0.1),
    "drain": dict(n_obj=600, n_scenes=2, groups_per_scene=6, players_per_group=3, n_ticks=48, seed=12,
                  destroy_frac=0.02, switch_frac=0.2, switch_new_groups=True, obj_props=True, obj_set_frac=0.1,
                  ext_frac=0.05, host_ops=True),
    "burst": dict(n_obj=4000, n_scenes=2, groups_per_scene=6, players_per_group=4, n_ticks=12, seed=13,
                  spawn_frac=0.3, destroy_frac=0.3, switch_frac=0.02, ext_frac=0.02, host_ops=True, records=True,
                  rec_rows=8, rec_set_frac=0.02, rec_row_frac=0.02),
}
# the frames of tiny_groups the golden fixture keeps (tests/golden/gen_churn_golden.py)
GOLDEN_WORLD, GOLDEN_TICKS = "tiny_groups", 42

_cache = {}


def world(name, n_ticks=None):
    """the named world (generated once a process; callers do not write into it)"""
    key = (name, n_ticks)
    if key not in _cache:
        kw = dict(WORLDS[name], rec_float_op=False, rec_set_float=False)
        if n_ticks is not None:
            kw["n_ticks"] = n_ticks
        _cache[key] = workload.make_world(**kw)
    return _cache[key]


def truncated(w, n_ticks):
    """the workload cut to its first n_ticks frames (the calls of later windows are never reached, and
    an object born later is never created): what a replay holds after frame n_ticks - 1"""
    t = dict(w)
    t["cfg"] = np.array(w["cfg"]).copy()
    t["cfg"][7] = n_ticks
    t["tick_time"] = np.asarray(w["tick_time"])[:n_ticks].copy()
    return t


class Membership:
    """pairs: the (scene, group) pairs that ever have a member, sorted; counts [n_ticks][n_pairs]: the
    live objects of each pair after window t's calls; alive [n_ticks][N], pair_of [n_ticks][N] (index
    into pairs, -1 for an object not alive); reused [n_ticks][N]: the object is alive after window t
    and entered its pair (created or switched in) in a window after some object left that pair
    (destroyed or switched out) — with slack, such an object may sit in a slot another object held"""

    def __init__(self, pairs, counts, alive, pair_of, reused, joined):
        self.pairs, self.counts, self.alive, self.pair_of, self.reused = pairs, counts, alive, pair_of, reused
        self.joined = joined   # per window: the pairs objects entered, or None when nothing changed place

    def drained(self):
        """indices of the pairs that had members, then nobody, then members again"""
        out = []
        for p in range(len(self.pairs)):
            c = self.counts[:, p]
            seen = np.nonzero(c > 0)[0]
            if len(seen) and np.any(c[seen[0]:seen[-1]] == 0):
                out.append(p)
        return out

    def refilled_at(self, p):
        """the windows in which pair p goes from nobody to members after having had members before"""
        c = self.counts[:, p]
        had = np.maximum.accumulate(c) > 0
        return [t for t in range(1, len(c)) if c[t] > 0 and c[t - 1] == 0 and had[t - 1]]


def membership(w):
    """Replay the membership of a workload only: objects enter at `born` (the first n0 before frame 0)
    in their creation-time (scene, group), move with the SwitchScene calls (sw_*; sw_scene < 0 is the
    object's own cell) and leave at d_tick.  A window's order is creations, switches, destructions."""
    N = len(w["guid_head"])
    nt = int(w["cfg"][7])
    born = np.asarray(w["born"]) if "born" in w else np.full(N, -1, np.int32)
    scene, group = np.array(w["scene"], np.int64), np.array(w["group"], np.int64)
    pairs = set(zip(scene.tolist(), group.tolist()))
    sw_t = np.asarray(w["sw_tick"]) if "sw_tick" in w else np.zeros(0, np.int32)
    if len(sw_t):
        sel = np.asarray(w["sw_scene"]) >= 0
        pairs |= set(zip(np.asarray(w["sw_scene"])[sel].tolist(), np.asarray(w["sw_group"])[sel].tolist()))
    pairs = sorted(pairs)
    index = {p: i for i, p in enumerate(pairs)}
    alive = np.zeros(N, bool)
    left = np.zeros(len(pairs), bool)      # somebody left the pair in an earlier window
    reused = np.zeros(N, bool)
    counts = np.zeros((nt, len(pairs)), np.int64)
    alive_t, pair_t, reused_t = np.zeros((nt, N), bool), np.full((nt, N), -1, np.int64), np.zeros((nt, N), bool)
    d_t = np.asarray(w["d_tick"]) if "d_tick" in w else np.zeros(0, np.int32)
    joined = []
    for t in range(nt):
        leaving, entering = [], []
        new = np.nonzero(born == t)[0] if t else np.nonzero(born <= 0)[0]
        alive[new] = True
        for o in new:
            reused[o] = left[index[(int(scene[o]), int(group[o]))]]
            entering.append(index[(int(scene[o]), int(group[o]))])
        for i in np.nonzero(sw_t == t)[0]:
            o, sc, gr = int(w["sw_obj"][i]), int(w["sw_scene"][i]), int(w["sw_group"][i])
            if sc < 0 or (sc, gr) == (int(scene[o]), int(group[o])):
                continue
            assert alive[o]
            leaving.append(index[(int(scene[o]), int(group[o]))])
            scene[o], group[o] = sc, gr
            reused[o] = left[index[(sc, gr)]]
            entering.append(index[(sc, gr)])
        for o in np.asarray(w["d_obj"])[d_t == t] if len(d_t) else ():
            assert alive[o]
            alive[o] = False
            leaving.append(index[(int(scene[o]), int(group[o]))])
        left[leaving] = True
        joined.append(set(entering) if t and (entering or leaving) else None)
        for o in np.nonzero(alive)[0]:
            p = index[(int(scene[o]), int(group[o]))]
            counts[t, p] += 1
            pair_t[t, o] = p
        alive_t[t] = alive
        reused_t[t] = reused & alive
    return Membership(pairs, counts, alive_t, pair_t, reused_t, joined)


def relayouts(w, slack_per_256):
    """(n_full, n_seg) a run must report (membership_stats()), by the layout's rule: a
    (scene, group) pair with members is a segment of members + slack slots, the slack max(2,
    ceil(members * slack / 256)) at the time of the last full layout (slack 0: the default 16 per 256, -1:
    none); a window whose calls move nobody counts as neither; one that brings a member to a pair without a
    segment (new, or empty at the last full layout) or more members to a segment than it has slots lays
    the world out again (full); any other rewrites the changed segments (seg)."""
    slack = 16 if slack_per_256 == 0 else max(slack_per_256, 0)
    room = lambda n: n + (0 if slack <= 0 else max(2, -(-n * slack // 256)))
    ms = membership(w)
    layout = lambda t: {p: room(int(n)) for p, n in enumerate(ms.counts[t]) if n > 0}
    cap = layout(0)
    n_full = n_seg = 0
    for t in range(1, len(ms.counts)):
        if ms.joined[t] is None:
            continue
        if any(p not in cap for p in ms.joined[t]) or any(ms.counts[t, p] > c for p, c in cap.items()):
            cap = layout(t)
            n_full += 1
        else:
            n_seg += 1
    return n_full, n_seg
