"""GPU: resource calls — nfk_adjust_props (NFCPropertyModule's AddHP / ConsumeHP / EnoughHP / AddMoney /
FullHPMP ..., PM:215-472) against tests/resource_call_model.py: every op at its edges on a hand-loaded
8-object world, on a clean window (k_adjust) and mid-window (the host path); batches of 0, 1, 255, 257
and 70001 calls whose (object, dst) groups chain and straddle blocks, by NFGUID and by object index; a
group longer than a block, interleaved dsts and a bound that is an earlier call's dst; twin worlds over
a workload with heartbeats and a linked record, one making adjust batches and one spelling every call out
as get_props / set_props, bit-equal frame by frame on both k_tick paths; every refusal; and the C++ plugin's
seventeen named methods over the golden script recorded from the compiled reference."""
import json
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import kernel, workload
from noahgameframe_amd.kernel import NFKError
from tests import resource_call_model as rcm
from tests.parity import ROOT

pytestmark = pytest.mark.gpu

PID = workload.PID
N_INT, N_FLT = workload.N_INT, workload.N_FLT
PRIVATE = workload.PRIVATE
T0 = 1_700_000_000_000
M64 = (1 << 64) - 1
HP, MAXHP, MP, MAXMP, SP, MAXSP, GOLD, MONEY = (PID[n] for n in ("HP", "MAXHP", "MP", "MAXMP", "SP", "MAXSP", "Gold", "EXP"))
EIGHT = [HP, MAXHP, MP, MAXMP, SP, MAXSP, GOLD, MONEY]
# the (op, dst, bound) shapes the named methods make, on this world's property ids (EXP stands for Money)
SHAPES = [(rcm.GAIN_ALIVE, HP, MAXHP), (rcm.SPEND_ALIVE, HP, -1), (rcm.ENOUGH, HP, -1), (rcm.FILL, HP, MAXHP),
          (rcm.GAIN_CAP, MP, MAXMP), (rcm.SPEND_ALIVE, MP, -1), (rcm.ENOUGH, MP, -1), (rcm.FILL, MP, MAXMP),
          (rcm.GAIN_CAP, SP, MAXSP), (rcm.SPEND_ALIVE, SP, -1), (rcm.FILL, SP, MAXSP),
          (rcm.GAIN, GOLD, -1), (rcm.SPEND, GOLD, -1), (rcm.ENOUGH, GOLD, -1), (rcm.GAIN, MONEY, -1), (rcm.SPEND, MONEY, -1)]
B62 = 1 << 62


def u64(v):
    return int(v) & M64


class Hand:
    """A hand-loaded world of n objects in 3 scene groups, no heartbeat scheduled: a frame only applies
    the queued calls.  world: the model's {(object, pid): value} of the eight properties."""

    def __init__(self, n, init=None, seed=1, committed=True):
        rng = np.random.default_rng(seed)
        self.n = n
        self.m = m = kernel.NFKernelModule(n + 8, n_class=2, n_rec=1)
        for c in range(2):
            m.set_prop_flags(c, workload._prop_flags()[c])
        m.define_record(0, 7, 3, [0, 0, 0], [PRIVATE, PRIVATE])
        self.gh = np.full(n, 7, np.int64)
        self.gd = np.arange(1, n + 1, dtype=np.int64) * 3
        self.cls = (np.arange(n) % 2).astype(np.uint8)
        m.create_objects(self.gh, self.gd, np.ones(n, np.int32), 1 + np.arange(n, dtype=np.int32) % 3, self.cls, self.cls)
        self.world = {}
        for p in EIGHT:
            if init is not None:
                col = np.array([init[o].get(p, 0) for o in range(n)], np.int64)
            elif p in (MAXHP, MAXMP, MAXSP):
                col = rng.integers(0, 60, n).astype(np.int64)
            else:
                col = rng.integers(-5, 80, n).astype(np.int64)
            m.load_prop(p, col)
            for o in range(n):
                self.world[(o, p)] = int(col[o])
        m.load_record(0, np.zeros((n, 3, 7), np.uint64), np.full(n, 0x7F, np.uint64))
        if committed:
            m.commit()
        self.t = 0

    def adjust(self, calls, by_obj=False, stats=None):
        """the batch on the device -> its result bytes; the model is not touched"""
        o = np.array([c[0] for c in calls], np.int64)
        a = ([c[1] for c in calls], [c[2] for c in calls], [c[3] for c in calls], [rcm.s64(c[4]) for c in calls])
        if by_obj:
            return self.m.adjust_props_obj(o.astype(np.int32), *a, stats=stats).tolist()
        return self.m.adjust_props(self.gh[o], self.gd[o], *a, stats=stats).tolist()

    def frame(self):
        self.t += 100
        self.m.Execute(T0 + self.t)
        return self.m.read_tick()

    def check_props(self, tag):
        for p in EIGHT:
            assert self.m.read_prop(p).tolist() == [self.world[(o, p)] for o in range(self.n)], (tag, "property", p)

    def check_frame(self, start, tag):
        """the frame's property events: per cell one event from the frame-start value to the final
        one, none when equal — what the equivalent SetPropertyInt calls raise.  (Expected from the
        model, not from a run of those calls: test_twin_worlds is the one that compares frames with a
        world that makes the spelled-out get_props / set_props calls.)"""
        t = self.frame()
        got = sorted((int(o), int(p), rcm.s64(int(a)), rcm.s64(int(b)))
                     for o, p, a, b in zip(t["ev_obj"], t["ev_pid"], t["ev_old"], t["ev_new"]))
        want = sorted((o, p, start[(o, p)], v) for (o, p), v in self.world.items() if start[(o, p)] != v)
        assert got == want, (tag, "events")
        self.check_props(tag)
        return want


# ---- edges ----
EDGE_INIT = [
    {HP: 60, MAXHP: 100},
    {HP: 100, MAXHP: 40},
    {MP: 0, MAXMP: 50, SP: 30, MAXSP: 30},
    {GOLD: 0, MONEY: 0},
    {HP: 5, MAXHP: 90, MP: 7, MAXMP: 0, SP: 1, MAXSP: -4},
    {HP: -B62, MAXHP: B62, MP: -B62, MAXMP: B62 - 1, GOLD: -B62, SP: B62, MAXSP: 2 * B62 - 1},
    {HP: 1, MAXHP: 2 * B62 - 1, GOLD: B62},
    {HP: 9, MAXHP: 9, MP: 9, MAXMP: 9, SP: 9, MAXSP: 9, GOLD: 9, MONEY: 9},
]
EDGE_CALLS = (
    # AddHP: below, exactly to and past MAXHP; v <= 0; Enough / Consume at and one past 0; HP == 0
    [(0, rcm.GAIN_ALIVE, HP, MAXHP, 10), (0, rcm.GAIN_ALIVE, HP, MAXHP, 30), (0, rcm.GAIN_ALIVE, HP, MAXHP, 500),
     (0, rcm.GAIN_ALIVE, HP, MAXHP, 0), (0, rcm.GAIN_ALIVE, HP, MAXHP, -5), (0, rcm.ENOUGH, HP, -1, 100),
     (0, rcm.ENOUGH, HP, -1, 101), (0, rcm.SPEND_ALIVE, HP, -1, 101), (0, rcm.SPEND_ALIVE, HP, -1, 100),
     (0, rcm.GAIN_ALIVE, HP, MAXHP, 5), (0, rcm.ENOUGH, HP, -1, 0), (0, rcm.SPEND_ALIVE, HP, -1, 0),
     (0, rcm.FILL, HP, MAXHP, 77)] +
    # MAXHP < HP: AddHP lowers HP; a negative Consume raises HP past MAXHP, by 2^62 too
    [(1, rcm.GAIN_ALIVE, HP, MAXHP, 1), (1, rcm.SPEND_ALIVE, HP, -1, -1000), (1, rcm.SPEND_ALIVE, HP, -1, -B62),
     (1, rcm.ENOUGH, HP, -1, B62 + 1040), (1, rcm.ENOUGH, HP, -1, B62 + 1041), (1, rcm.GAIN_ALIVE, HP, MAXHP, 1)] +
    # AddMP on MP == 0 raises it; caps; Consume one past 0, then to exactly 0
    [(2, rcm.GAIN_CAP, MP, MAXMP, 7), (2, rcm.GAIN_CAP, MP, MAXMP, 1000), (2, rcm.SPEND_ALIVE, MP, -1, 51),
     (2, rcm.SPEND_ALIVE, MP, -1, 50), (2, rcm.SPEND_ALIVE, MP, -1, 1), (2, rcm.GAIN_CAP, MP, MAXMP, -1),
     (2, rcm.SPEND_ALIVE, SP, -1, 30), (2, rcm.GAIN_CAP, SP, MAXSP, 4), (2, rcm.FILL, SP, MAXSP, 0)] +
    # Gold == 0: EnoughMoney(0) is false; ConsumeMoney(0), AddMoney(-1); sums up to 2^63 - 1
    [(3, rcm.ENOUGH, GOLD, -1, 0), (3, rcm.SPEND, GOLD, -1, 1), (3, rcm.GAIN, GOLD, -1, -1), (3, rcm.GAIN, GOLD, -1, B62),
     (3, rcm.GAIN, GOLD, -1, B62 - 1), (3, rcm.SPEND, GOLD, -1, 0), (3, rcm.ENOUGH, GOLD, -1, 2 * B62 - 1),
     (3, rcm.SPEND, GOLD, -1, 2 * B62 - 1), (3, rcm.SPEND, GOLD, -1, 1), (3, rcm.GAIN, MONEY, -1, 3),
     (3, rcm.SPEND, MONEY, -1, 4), (3, rcm.SPEND, MONEY, -1, 3), (3, rcm.ENOUGH, MONEY, -1, 0)] +
    # FullHPMP with MAXMP == 0: HP is filled, MP is left alone; a negative maximum fills nothing
    [(4, rcm.FILL, HP, MAXHP, 0), (4, rcm.FILL, MP, MAXMP, 0), (4, rcm.FILL, SP, MAXSP, 0), (4, rcm.GAIN_CAP, SP, MAXSP, 2)] +
    # values near -2^62 and 2^62, no overflow
    [(5, rcm.ENOUGH, HP, -1, -B62), (5, rcm.SPEND_ALIVE, HP, -1, -B62), (5, rcm.GAIN_ALIVE, HP, MAXHP, B62),
     (5, rcm.GAIN_CAP, MP, MAXMP, B62), (5, rcm.GAIN_CAP, MP, MAXMP, B62), (5, rcm.SPEND, GOLD, -1, B62),
     (5, rcm.GAIN, GOLD, -1, B62), (5, rcm.GAIN, GOLD, -1, B62), (5, rcm.GAIN_CAP, SP, MAXSP, B62 - 2),
     (5, rcm.GAIN_CAP, SP, MAXSP, 1), (5, rcm.SPEND_ALIVE, SP, -1, 2 * B62 - 1), (5, rcm.ENOUGH, MP, -1, -B62)] +
    [(6, rcm.GAIN_ALIVE, HP, MAXHP, 2 * B62 - 2), (6, rcm.ENOUGH, HP, -1, 2 * B62 - 1), (6, rcm.SPEND, GOLD, -1, B62),
     (6, rcm.SPEND_ALIVE, HP, -1, -0), (6, rcm.SPEND_ALIVE, HP, -1, 2 * B62 - 2)] +
    # every shape back to back on one object
    [(7, op, d, b, 3) for op, d, b in SHAPES])


@pytest.mark.parametrize("mid_window", [False, True])
def test_edges(gpu_available, mid_window):
    h = Hand(8, init=EDGE_INIT)
    try:
        start = dict(h.world)
        if mid_window:      # Sets queued first: every call's cells have pending state, the host answers
            # (the values move away and back, so the calls meet the same states through the queue)
            cells = sorted(h.world)
            o = np.array([c[0] for c in cells])
            for bump in (17, 0):
                h.m.set_props(h.gh[o], h.gd[o], [c[1] for c in cells], [u64(h.world[c] + bump) for c in cells])
        want, sets = rcm.adjust(h.world, list(EDGE_CALLS))
        st = {}
        got = h.adjust(EDGE_CALLS, stats=st)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (k, EDGE_CALLS[k], g, w)
        n = len(EDGE_CALLS)
        assert (st["n_host"], st["n_dev"]) == ((n, 0) if mid_window else (0, n)), st
        assert st["n_set"] == len(sets) > 40
        assert st["bytes"] == (0 if mid_window else (9 * n + 15) // 16 * 16)   # 8 + 1 bytes a call, one copy
        # mid-window reads see the batch's Sets
        cells = sorted(h.world)
        o = np.array([c[0] for c in cells])
        now = h.m.get_props(h.gh[o], h.gd[o], [c[1] for c in cells]).view(np.int64).tolist()
        assert now == [h.world[c] for c in cells]
        ev = h.check_frame(start, "edges")
        assert len(ev) >= 8      # (the model's count: the cells whose final value differs from the frame's start)
        # the next window is clean again: the kernel answers
        start = dict(h.world)
        want, _ = rcm.adjust(h.world, list(EDGE_CALLS))
        assert h.adjust(EDGE_CALLS, stats=st) == want and st["n_host"] == 0
        h.check_frame(start, "edges again")
    finally:
        h.m.close()


# ---- batch sizes ----
def _random_calls(rng, n, objects):
    sh = rng.integers(0, len(SHAPES), n)
    ob = rng.choice(objects, n)
    vs = np.where(rng.random(n) < 0.1, rng.integers(-3, 1, n), rng.integers(1, 40, n))
    return [(int(o), *SHAPES[s], int(v)) for o, s, v in zip(ob, sh, vs)]


@pytest.fixture(scope="module")
def batch_calls():
    rng = np.random.default_rng(7)
    return {n: _random_calls(rng, n, np.arange(300)) for n in (0, 1, 255, 257, 70001)}


@pytest.mark.parametrize("n", [0, 1, 255, 257, 70001])
def test_batch_sizes(gpu_available, batch_calls, n):
    """objects and dsts repeat: groups chain within the batch and straddle block boundaries; 70001
    calls grow the staging buffers (the batches before it on this world are small)"""
    h = Hand(300, seed=n + 1)
    try:
        start = dict(h.world)
        small = batch_calls[1]
        want, _ = rcm.adjust(h.world, small)
        assert h.adjust(small) == want          # (a first, small batch: the buffers start small)
        h.check_frame(start, "small")
        start = dict(h.world)
        calls = batch_calls[n]
        want, sets = rcm.adjust(h.world, list(calls))
        st = {}
        got = h.adjust(calls, stats=st)
        assert got == want
        assert (st["n_dev"], st["n_host"], st["n_set"]) == (n, 0, len(sets)), st
        h.check_frame(start, f"n = {n}")
    finally:
        h.m.close()


def test_by_object_index_equals_by_guid(gpu_available, batch_calls):
    """the _obj form fed from nfk_query_objects' hits"""
    a, b = Hand(300, seed=3), Hand(300, seed=3)
    try:
        hits = b.m.query_objects([kernel.query(1, who=kernel.Q_PLAYERS), kernel.query(1, who=kernel.Q_OTHERS)])
        objs = np.concatenate([np.asarray(x, np.int64) for x in hits])
        assert sorted(objs.tolist()) == list(range(300))
        rng = np.random.default_rng(11)
        for w in range(2):
            calls = _random_calls(rng, 2000, objs[: 200 + 100 * w])
            sa, sb = {}, {}
            ra, rb = a.adjust(calls, stats=sa), b.adjust(calls, by_obj=True, stats=sb)
            want, _ = rcm.adjust(a.world, list(calls))
            assert ra == rb == want
            assert sa == {**sb, "kernel_ms": sa["kernel_ms"]} and sa["n_host"] == 0
            ta, tb = a.frame(), b.frame()
            for k in ("ev_obj", "ev_pid", "ev_old", "ev_new", "mo_off", "mr_obj"):
                assert np.array_equal(ta[k], tb[k]), k
            a.check_props(f"window {w}")
        with pytest.raises(NFKError) as e:      # an index that is no live object
            b.m.adjust_props_obj([0, 300], [rcm.ENOUGH] * 2, [HP] * 2, [-1] * 2, [1, 1])
        assert e.value.code == -7
    finally:
        a.m.close()
        b.m.close()


# ---- group shapes ----
def test_group_shapes_in_one_batch(gpu_available):
    h = Hand(300, seed=5)
    try:
        rng = np.random.default_rng(13)
        start = dict(h.world)
        calls = _random_calls(rng, 300, np.arange(100, 300))
        # one object with 600 calls on one dst (a group longer than a block), the same object with three
        # more dsts interleaved
        hp = [s for s in SHAPES if s[1] == HP]
        other = [s for s in SHAPES if s[1] in (MP, SP, GOLD)]
        for k in range(600):
            calls.append((5, *hp[int(rng.integers(0, len(hp)))], int(rng.integers(-2, 30))))
            if k % 2:
                calls.append((5, *other[int(rng.integers(0, len(other)))], int(rng.integers(-2, 30))))
        # a call whose bound is an earlier (and a later) call's dst: those two groups go to the host
        calls += [(7, rcm.GAIN, MAXHP, -1, 5), (7, rcm.GAIN_ALIVE, HP, MAXHP, 1000), (7, rcm.GAIN, MAXHP, -1, 50),
                  (7, rcm.FILL, HP, MAXHP, 0), (7, rcm.SPEND_ALIVE, HP, -1, 3)]
        order = rng.permutation(len(calls) - 5)          # (the chains keep their order where it matters: shuffled
        calls = [calls[i] for i in sorted(order[:400])] + calls[-5:] + [calls[i] for i in sorted(order[400:])]   # stably)
        want, sets = rcm.adjust(h.world, list(calls))
        st = {}
        got = h.adjust(calls, stats=st)
        bad = [k for k in range(len(calls)) if got[k] != want[k]]
        assert not bad, (bad[:5], [calls[k] for k in bad[:5]])
        assert st["n_host"] == 5 and st["n_dev"] == len(calls) - 5 and st["n_set"] == len(sets), st
        assert h.world[(7, HP)] == h.world[(7, MAXHP)] - 3
        h.check_frame(start, "group shapes")
        # the same batch again in a window where object 5's HP has a queued Set: that group moves to the host
        start = dict(h.world)
        h.m.set_props(h.gh[5:6], h.gd[5:6], [HP], [u64(12)])
        h.world[(5, HP)] = 12
        want, _ = rcm.adjust(h.world, list(calls))
        assert h.adjust(calls, stats=st) == want
        assert st["n_host"] == 5 + sum(1 for c in calls if c[0] == 5 and c[2] == HP), st
        # and a third batch in the same window: every touched pair is pending now
        third = [c for c in calls if c[0] == 5][:50]
        want, _ = rcm.adjust(h.world, list(third))
        assert h.adjust(third, stats=st) == want and st["n_dev"] == 0
        h.check_frame(start, "group shapes, pending")
    finally:
        h.m.close()


# ---- twin worlds ----
def _twin_world(w):
    """kernel.world_from_workload with one more thing: record 0 (7 x 3 ints) linked to MAXHP, MAXMP,
    MAXSP, row 0 holding the creation-time maxima"""
    n_obj, n_int, n_flt, n_cls, n_kind = (int(x) for x in w["cfg"][:5])
    m = kernel.NFKernelModule(n_obj + 64, n_int, n_flt, n_cls, n_kind, 1)
    for c in range(n_cls):
        m.set_prop_flags(c, w["prop_flags"][c])
    m.define_record(0, 7, 3, [0, 0, 0], [PRIVATE] * n_cls)
    for k in range(n_kind):
        m.define_kind(k, w["ops"][k][: int(w["n_ops"][k])])
    m.link_record(0, 7, [MAXHP, MAXMP, MAXSP])
    m.create_objects(w["guid_head"], w["guid_data"], w["scene"], w["group"], w["cls"], w["is_player"])
    for p in range(n_int):
        m.load_prop(p, w["init_i"][p])
    for p in range(n_flt):
        m.load_prop(n_int + p, w["init_f"][p])
    cells = np.zeros((n_obj, 3, 7), np.uint64)
    for c, p in enumerate((MAXHP, MAXMP, MAXSP)):
        cells[:, c, 0] = w["init_i"][p].astype(np.int64).view(np.uint64)
    m.load_record(0, cells, np.full(n_obj, 0x7F, np.uint64))
    m.commit()
    so = w["s_obj"]
    m.add_schedules(w["guid_head"][so], w["guid_data"][so], w["s_kind"], w["s_interval"], w["s_count"], w["s_time"])
    return m


def _spelled_out(m, gh, gd, calls):
    """the contract's loop: every call as get_props / the rule / set_props, one call at a time"""
    rets = []
    for (o, op, dst, bound, v) in calls:
        g = ([gh[o]], [gd[o]])
        cur = int(m.get_props(*g, [dst]).view(np.int64)[0])
        mx = int(m.get_props(*g, [bound]).view(np.int64)[0]) if bound >= 0 else 0
        r, nv = rcm.rule(op, cur, mx, rcm.s64(v))
        if nv is not None:
            m.set_props(*g, [dst], [u64(nv)])
            r |= rcm.SET
        rets.append(r)
    return rets


@pytest.mark.parametrize("path", ["jit", "library"])
def test_twin_worlds(gpu_available, monkeypatch, path):
    """world A makes adjust_props batches, world B the same calls spelled out; everything else —
    heartbeat programs that move HP, MP (HPRegen, MPRegen, Poison clamp to the linked maxima), Sets,
    calls on the linked record, spawns, a destroy — is the same.  Frames bit-equal, every property equal."""
    if path == "library":
        monkeypatch.setenv("NFGPU_JIT", "0")
    w = workload.make_world(n_obj=600, n_scenes=2, groups_per_scene=4, players_per_group=3, n_ticks=5, seed=23)
    A, Bw = _twin_world(w), _twin_world(w)
    try:
        for m in (A, Bw):
            on, msg = m.jit_status()
            assert bool(on) == (path == "jit"), msg
        gh, gd = list(w["guid_head"]), list(w["guid_data"])
        alive = list(range(600))
        rng = np.random.default_rng(29)
        n_host = n_dev = n_ev = n_fi = 0
        for win in range(5):
            st = {}
            steps = []          # ("adjust", calls) or (method name, args): the window's calls in order
            for _ in range(int(rng.integers(5, 9))):
                k = int(rng.integers(0, 5))
                objs = rng.choice(alive, 150)
                if k == 0:      # Sets of unlinked properties, some of them the calls' dsts
                    p = rng.choice([HP, MP, GOLD, PID["Camp"]], 150)
                    steps.append(("set_props", ([gh[o] for o in objs], [gd[o] for o in objs], p, rng.integers(0, 900, 150).astype(np.uint64))))
                elif k == 1:    # the maxima move through the linked record
                    steps.append(("set_records", ([gh[o] for o in objs], [gd[o] for o in objs], [0] * 150, rng.integers(0, 7, 150),
                                                  rng.integers(0, 3, 150), rng.integers(0, 2000, 150).astype(np.uint64))))
                else:
                    calls = _random_calls(rng, int(rng.integers(1, 300)), alive)
                    calls = [(o, op, d, b, v * int(rng.choice([1, 1, 50, B62 // 64]))) for o, op, d, b, v in calls]
                    steps.append(("adjust", calls))
            if win in (1, 3):   # spawns, then calls on them; a destroy
                k = len(gh)
                props = np.zeros((2, N_INT + N_FLT), np.uint64)
                props[:, HP], props[:, MAXHP], props[:, GOLD] = 10, 50, 7
                steps.insert(1, ("spawn_objects", ([7, 7], [1 << 50 | k, 1 << 50 | (k + 1)], [1, 1], [1, 2], [0, 1], [0, 1], props)))
                gh += [7, 7]
                gd += [1 << 50 | k, 1 << 50 | (k + 1)]
                steps.insert(2, ("adjust", [(k, rcm.GAIN_ALIVE, HP, MAXHP, 100), (k + 1, rcm.SPEND, GOLD, -1, 7),
                                            (k, rcm.FILL, MP, MAXMP, 0), (3, rcm.ENOUGH, HP, -1, 1)]))
                alive += [k, k + 1]
                dead = alive.pop(17)
                steps.append(("destroy_objects", ([gh[dead]], [gd[dead]])))
            for name, args in steps:
                if name == "adjust":
                    ra = A.adjust_props([gh[c[0]] for c in args], [gd[c[0]] for c in args], [c[1] for c in args],
                                        [c[2] for c in args], [c[3] for c in args], [rcm.s64(c[4]) for c in args], stats=st).tolist()
                    assert ra == _spelled_out(Bw, gh, gd, args), (win, "results")
                    n_host += st["n_host"]
                    n_dev += st["n_dev"]
                else:
                    getattr(A, name)(*args)
                    getattr(Bw, name)(*args)
            now = T0 + 400 * (win + 1)
            A.Execute(now)
            Bw.Execute(now)
            ta, tb = A.read_tick(), Bw.read_tick()
            ta.pop("summary"), tb.pop("summary")
            assert sorted(ta) == sorted(tb)
            for k in ta:
                assert np.array_equal(ta[k], tb[k]), (win, k)
            for p in range(N_INT + N_FLT):
                assert np.array_equal(A.read_prop(p), Bw.read_prop(p)), (win, p)
            n_fi += len(ta["fi_obj"])       # (the schedules exist from the end of the first frame on)
            n_ev += len(ta["ev_obj"])
        assert n_host > 50 and n_dev > 50 and n_ev > 1000 and n_fi > 1000, (n_host, n_dev, n_ev, n_fi)
    finally:
        A.close()
        Bw.close()


# ---- errors ----
def _refused(fn, code):
    with pytest.raises(NFKError) as e:
        fn()
    assert e.value.code == code, e.value


def test_errors(gpu_available):
    """the code, nothing of the batch queued, the next batch answered"""
    h = Hand(20, seed=9, committed=False)
    try:
        m, gh, gd = h.m, h.gh, h.gd
        ok = ([rcm.GAIN, rcm.GAIN], [GOLD, GOLD], [-1, -1], [5, 6])
        _refused(lambda: m.adjust_props(gh[:2], gd[:2], *ok), -3)                                   # before commit
        m.link_record(0, 7, [PID["ATK_VALUE"], -1, -1])
        m.commit()

        def bad(o, op, dst, bound, code=-1):
            # (a good call in front of every bad one)
            _refused(lambda: m.adjust_props([gh[0], gh[o]], [gd[0], gd[o]], [rcm.GAIN, op], [GOLD, dst], [-1, bound], [5, 1]), code)
            _refused(lambda: m.adjust_props_obj([0, o], [rcm.GAIN, op], [GOLD, dst], [-1, bound], [5, 1]), code)
        _refused(lambda: m.adjust_props([gh[0], 7], [gd[0], 123456], *ok), -7)                      # an unknown NFGUID
        _refused(lambda: m.adjust_props_obj([0, 20], *ok), -7)
        _refused(lambda: m.adjust_props_obj([0, -1], *ok), -7)
        bad(1, rcm.GAIN, PID["X"], -1)                                                              # a float dst
        bad(1, rcm.GAIN, N_INT + N_FLT, -1)                                                         # no such property
        bad(1, rcm.GAIN, -1, -1)
        bad(1, rcm.GAIN, PID["ATK_VALUE"], -1)                                                      # a linked dst
        bad(1, rcm.GAIN, GOLD, MAXHP)                                                               # a bound where the op takes none
        bad(1, rcm.SPEND_ALIVE, HP, MAXHP)
        bad(1, rcm.SPEND, GOLD, MAXHP)
        bad(1, rcm.ENOUGH, HP, MAXHP)
        for op in (rcm.GAIN_ALIVE, rcm.GAIN_CAP, rcm.FILL):
            bad(1, op, HP, -1)                                                                      # and the reverse
            bad(1, op, HP, PID["X"])                                                                # a float bound
            bad(1, op, HP, N_INT + N_FLT)
        bad(1, 7, HP, -1)                                                                           # a bad op
        bad(1, 255, HP, MAXHP)
        assert m.lib.nfk_adjust_props(m.h, 1, None, None, None, None, None, None, None) == -1       # null arguments
        assert m.lib.nfk_adjust_props(m.h, -1, None, None, None, None, None, None, None) == -1
        assert m.lib.nfk_adjust_stats(m.h, None) == -1
        # an object destroyed in the window
        m.destroy_objects(gh[19:20], gd[19:20])
        bad(19, rcm.GAIN, GOLD, -1, code=-7)
        # nothing of any refused batch was queued; a linked bound is fine; the next batch is answered
        st = {}
        assert m.get_props(gh[:1], gd[:1], [GOLD]).view(np.int64)[0] == h.world[(0, GOLD)]
        calls = [(0, rcm.GAIN, GOLD, -1, 5), (1, rcm.GAIN_CAP, HP, PID["ATK_VALUE"], 1 << 40)]
        h.world[(1, PID["ATK_VALUE"])] = 0
        m.set_records(gh[1:2], gd[1:2], [0], [2], [0], [u64(33)])     # the linked bound moves in this window: host
        h.world[(1, PID["ATK_VALUE"])] = 33
        want, _ = rcm.adjust(h.world, calls)
        assert h.adjust(calls, stats=st) == want and (st["n_dev"], st["n_host"], st["n_set"]) == (1, 1, 2)
        t = h.frame()
        ev = sorted(zip(t["ev_obj"].tolist(), t["ev_pid"].tolist(), t["ev_new"].view(np.int64).tolist()))
        assert ev == [(0, GOLD, h.world[(0, GOLD)]), (1, HP, 33), (1, PID["ATK_VALUE"], 33)], ev
    finally:
        h.m.close()


def test_errors_object_property(gpu_available):
    """a world that has object (NFGUID) properties: one as dst is refused as nfk_set_props refuses it,
    one as bound is no int property; by NFGUID and by object index; nothing of the batch queued, the
    next batch answered"""
    n, n_op = 12, 3
    m = kernel.NFKernelModule(n + 8, n_class=2, n_rec=0, n_oprops=n_op)
    try:
        for c in range(2):
            m.set_prop_flags(c, workload._prop_flags(n_op)[c])
        gh, gd = np.full(n, 7, np.int64), np.arange(1, n + 1, dtype=np.int64) * 5
        cls = (np.arange(n) % 2).astype(np.uint8)
        m.create_objects(gh, gd, np.ones(n, np.int32), np.ones(n, np.int32), cls, cls)
        m.load_prop(GOLD, np.full(n, 40, np.int64))
        m.load_prop(HP, np.full(n, 10, np.int64))
        m.load_prop(MAXHP, np.full(n, 30, np.int64))
        for p in range(n_op):
            m.load_object(N_INT + N_FLT + p, np.zeros(n, np.int64), np.zeros(n, np.int64))
        m.commit()
        world = {(o, p): v for o in range(n) for p, v in ((GOLD, 40), (HP, 10), (MAXHP, 30))}
        for oprop in (N_INT + N_FLT, N_INT + N_FLT + n_op - 1):
            for op, dst, bound in ((rcm.GAIN, oprop, -1), (rcm.ENOUGH, oprop, -1), (rcm.FILL, oprop, MAXHP),
                                   (rcm.GAIN_ALIVE, HP, oprop), (rcm.GAIN_CAP, HP, oprop), (rcm.FILL, HP, oprop)):
                # (a good call in front of the bad one)
                _refused(lambda: m.adjust_props(gh[:2], gd[:2], [rcm.GAIN, op], [GOLD, dst], [-1, bound], [5, 1]), -1)
                _refused(lambda: m.adjust_props_obj([0, 1], [rcm.GAIN, op], [GOLD, dst], [-1, bound], [5, 1]), -1)
        with pytest.raises(NFKError) as e:
            m.adjust_props(gh[:1], gd[:1], [rcm.GAIN], [N_INT + N_FLT], [-1], [1])
        assert "object property" in str(e.value)
        _refused(lambda: m.adjust_props(gh[:1], gd[:1], [rcm.GAIN], [N_INT + N_FLT + n_op], [-1], [1]), -1)   # past the last one
        assert m.get_props(gh[:2], gd[:2], [GOLD, GOLD]).view(np.int64).tolist() == [40, 40]    # nothing was queued
        calls = [(0, rcm.GAIN, GOLD, -1, 5), (1, rcm.GAIN_ALIVE, HP, MAXHP, 100), (0, rcm.SPEND, GOLD, -1, 45)]
        want, sets = rcm.adjust(world, calls)
        st = {}
        got = m.adjust_props(gh[[0, 1, 0]], gd[[0, 1, 0]], [c[1] for c in calls], [c[2] for c in calls],
                             [c[3] for c in calls], [c[4] for c in calls], stats=st).tolist()
        assert got == want and (st["n_dev"], st["n_host"], st["n_set"]) == (3, 0, len(sets))
        m.Execute(T0 + 100)
        t = m.read_tick()
        ev = sorted(zip(t["ev_obj"].tolist(), t["ev_pid"].tolist(), t["ev_old"].view(np.int64).tolist(),
                        t["ev_new"].view(np.int64).tolist()))
        assert ev == [(0, GOLD, 40, 0), (1, HP, 10, 30)], ev
    finally:
        m.close()


# ---- the C++ plugin ----
def test_cpp_plugin(gpu_available, tmp_path):
    """NFGPUKernelModule's seventeen named methods over the golden script, call for call against the
    answers recorded from the compiled NFCPropertyModule: the return values and the object's eight
    properties right after each call (mid-window), every object's after each frame, and the frames'
    property events against the model's window rule"""
    with open(os.path.join(ROOT, "tests", "golden", "resource_calls.json")) as f:
        g = json.load(f)
    script, answers = g["script"], g["answers"]
    sp = tmp_path / "script.txt"
    sp.write_text("\n".join(script) + "\n")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "_bin", "resource_calls_plugin"), str(sp)], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got, frames, got_ev = [], {}, {}
    for ln in run.stdout.splitlines():
        f = ln.split(":")[0].split()
        if ln.startswith("A "):
            assert int(f[1]) == len(got), ln
            got.append([int(f[2]), [int(x) for x in ln.split(":")[1].split()]])
        elif ln.startswith("F "):
            frames[(int(f[1]), int(f[2]))] = [int(x) for x in ln.split(":")[1].split()]
        elif ln.startswith("P "):
            f = ln.split()
            got_ev.setdefault((int(f[1]), int(f[2])), []).append((f[3], int(f[4]), int(f[5])))
    calls = [ln for ln in script if ln.split()[0] not in ("BASE", "OBJ", "X")]
    assert len(got) == len(answers) == len(calls)
    for k, (a, b) in enumerate(zip(got, answers)):
        assert a == b, (k, calls[k], a, b)
    # after every frame: the reference's last recorded state of each object, and the window's events
    state = {o: None for o in range(rcm.GOLDEN_OBJECTS)}
    begin, win, k, n_ev = {}, 0, 0, 0
    created = rcm.Player(rcm.GOLDEN_BASE)
    for o in state:
        state[o] = [created.props[n] for n in rcm.PROPS]
        begin[o] = list(state[o])
    for ln in script:
        f = ln.split()
        if f[0] in ("BASE", "OBJ"):
            continue
        if f[0] == "X":
            for o in state:
                assert frames[(win, o)] == state[o], (win, o)
                want = sorted((rcm.PROPS[i], begin[o][i], state[o][i]) for i in range(8) if begin[o][i] != state[o][i])
                assert sorted(got_ev.get((win, o), [])) == want, (win, o)
                n_ev += len(want)
                begin[o] = list(state[o])
            win += 1
            continue
        if int(f[1]) in state:
            state[int(f[1])] = answers[k][1]
        k += 1
    assert win == script.count("X") and n_ev > 15
