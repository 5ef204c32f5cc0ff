"""GPU: property links — nfk_link_record (NFCPropertyModule::OnRecordPropertyEvent, PM:127-149)
against tests/record_link_model.py: random windows of every record call on a 7 x 16 record over 300
objects in 3 scene groups (the frame's property events with their recipients, the columns, the
records), the same against a twin world that has no links and is handed the model's final values as
direct Sets, a 64 x 3 record summed over all 64 rows and one summed over its first row, mid-window
reads, a heartbeat program clamping HP to a linked MAXHP on the three k_tick paths, the calls-only
pass, every refusal, a world whose links see no call, and the C++ plugin's LinkRecordColumns over the
golden script recorded from the compiled reference."""
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import kernel, workload
from noahgameframe_amd.kernel import NFKError
from tests import record_link_model as rlm
from tests.parity import ROOT
from tests.record_link_model import LinkRecord

pytestmark = pytest.mark.gpu

PID = workload.PID
N_INT, N_FLT = workload.N_INT, workload.N_FLT
PUBLIC, PRIVATE, UPLOAD = workload.PUBLIC, workload.PRIVATE, workload.UPLOAD
T0 = 1_700_000_000_000
M64 = (1 << 64) - 1

# the 7 x 16 record: every int property but SceneID / GroupID hangs on a column, in no particular order;
# column 5 has no link
COLS16 = [PID["MAXHP"], PID["ATK_VALUE"], PID["DEF_VALUE"], PID["MAXMP"], PID["MAXSP"], -1, PID["HPREGEN"],
          PID["MPREGEN"], PID["SPREGEN"], PID["EXP"], PID["Gold"], PID["Level"], PID["Camp"], PID["NPCType"],
          PID["HP"], PID["MP"]]


def u64(v):
    return int(v) & M64


class LHand:
    """A hand-loaded world: record 0 with a link (or, link=False, the same world without it: the
    twin), record 1 (4 x 3) without one; per object the model's LinkRecord of record 0.  No heartbeat
    is scheduled unless a test adds one, so a frame only applies the queued calls."""

    def __init__(self, n, rows, cols, rows_l, col_pid, seed, link=True, kinds=None, before_commit=None):
        rng = np.random.default_rng(seed)
        self.n, self.rows, self.cols, self.col_pid = n, rows, cols, list(col_pid)
        self.m = m = kernel.NFKernelModule(n + 8, n_class=2, n_rec=2)
        self.flags = workload._prop_flags()
        for c in range(2):
            m.set_prop_flags(c, self.flags[c])
        m.define_record(0, rows, cols, [0] * cols, [PRIVATE, PRIVATE])
        m.define_record(1, 4, 3, [0, 0, 0], [PRIVATE, PRIVATE])
        for k, ops in (kinds or {}).items():
            m.define_kind(k, np.array(ops, workload.OP_DTYPE))
        if link:
            m.link_record(0, rows_l, col_pid)
        self.gh = np.full(n, 7, np.int64)
        self.gd = np.arange(1, n + 1, dtype=np.int64) * 3
        self.cls = (np.arange(n) % 2).astype(np.uint8)
        self.group = 1 + np.arange(n, dtype=np.int32) % 3
        m.create_objects(self.gh, self.gd, np.ones(n, np.int32), self.group, self.cls, self.cls)
        self.pids = sorted(p for p in col_pid if p >= 0)
        init = {p: rng.integers(-50, 50, n).astype(np.int64) for p in self.pids}
        for p in self.pids:
            m.load_prop(p, init[p])
        cells = np.zeros((n, cols, rows), np.uint64)
        used = np.zeros(n, np.uint64)
        self.rec = []
        for o in range(n):
            r = LinkRecord(rows, cols, rows_l, col_pid, props={p: int(init[p][o]) for p in self.pids})
            r.used = int(rng.integers(0, 1 << min(rows, 62))) | (int(rng.integers(0, 4)) << max(rows - 2, 0))
            r.used &= (1 << rows) - 1
            if o == 1:
                r.used = 0
            if o == 2:
                r.used = (1 << rows) - 1
            for c in range(cols):
                for row in range(rows):
                    r.cells[c][row] = int(rng.integers(-9, 10))
                    cells[o, c, row] = u64(r.cells[c][row])
            used[o] = r.used
            self.rec.append(r)
        m.load_record(0, cells, used)
        m.load_record(1, np.zeros((n, 3, 4), np.uint64), np.full(n, 0b11, np.uint64))
        if before_commit:
            before_commit(self)
        m.commit()
        self.t = 0

    def g(self, o):
        return [self.gh[o]], [self.gd[o]]

    def call(self, o, call, rec=0, model=True):
        """one record call queued on the device and applied to the model"""
        m, (gh, gd) = self.m, self.g(o)
        k = call[0]
        if k == "set":
            m.set_records(gh, gd, [rec], [call[1]], [call[2]], [u64(call[3])])
        elif k == "add":
            vals = None if call[2] is None else [[u64(v) for v in call[2]] + [0] * (16 - len(call[2]))]
            m.record_rows(gh, gd, [rec], [1], [call[1]], vals)
        elif k == "rm":
            m.record_rows(gh, gd, [rec], [2], [call[1]])
        elif k == "swap":
            m.swap_rows(gh, gd, [rec], [call[1]], [call[2]])
        else:
            m.record_rows(gh, gd, [rec], [3], [0])
        if model and rec == 0:
            self.rec[o].apply(call)

    def want_events(self):
        """{object: [(pid, old, new)]} of the window, the models' window memories ended"""
        want = {}
        for o in range(self.n):
            ev = self.rec[o].frame_events()
            if ev:
                want[o] = ev
        return want

    def recipients(self, o, pid):
        f = int(self.flags[self.cls[o]][pid])
        if f & PUBLIC:
            return [x for x in range(self.n) if self.cls[x] and self.group[x] == self.group[o] and x != o]
        if (f & PRIVATE) and not (f & UPLOAD):
            return [o]
        return []

    def frame(self, calls_only=False):
        self.t += 100
        if calls_only:
            self.m.ExecuteCalls()
        else:
            self.m.Execute(T0 + self.t)
        return self.m.read_tick()

    def check_frame(self, tag, calls_only=False, want=None):
        """the frame's property events per object in order, with their recipients; the linked
        properties' columns; the record"""
        want = self.want_events() if want is None else want
        t = self.frame(calls_only)
        got, rcpt = {}, {}
        for i in range(len(t["ev_obj"])):
            o, pid = int(t["ev_obj"][i]), int(t["ev_pid"][i])
            got.setdefault(o, []).append((pid, rlm.s64(int(t["ev_old"][i])), rlm.s64(int(t["ev_new"][i]))))
            a, b = int(t["mo_off"][i]), int(t["mo_off"][i + 1])
            rcpt.setdefault(o, []).append(sorted(int(x) for x in t["mr_obj"][a:b]))
        assert sorted(got) == sorted(want), f"{tag}: objects with property events"
        for o in want:
            assert got[o] == want[o], (tag, o)
            assert rcpt[o] == [self.recipients(o, e[0]) for e in want[o]], (tag, o, "recipients")
        self.check_state(tag)
        return t, want

    def check_state(self, tag):
        for p in self.pids:
            dev = self.m.read_prop(p)
            assert dev.tolist() == [self.rec[o].props[p] for o in range(self.n)], (tag, "property", p)
        um = self.m.get_used_rows(self.gh, self.gd, np.zeros(self.n, np.int32))
        assert [int(x) for x in um] == [r.used for r in self.rec], (tag, "used rows")
        dev = self.m.read_record(0)
        for o in range(self.n):
            r = self.rec[o]
            for row in range(self.rows):
                if r.is_used(row):
                    assert [int(x) for x in dev[o][:, row]] == [u64(r.cells[c][row]) for c in range(self.cols)], (tag, o, row)


def _random_window(h, rng, touched, lo=1, hi=9, twin=None):
    for o in touched:
        for _ in range(int(rng.integers(lo, hi))):
            c = rlm.random_call(rng, h.rec[o])
            h.call(o, c)
            if twin is not None:
                twin.call(o, c, model=False)


def _same_frame(ta, tb, tag):
    ev = [sorted(zip(t["ev_obj"].tolist(), t["ev_pid"].tolist(), t["ev_old"].tolist(), t["ev_new"].tolist())) for t in (ta, tb)]
    assert ev[0] == ev[1], (tag, "property events", sorted(set(ev[0]) ^ set(ev[1]))[:6])
    for k in ("ev_obj", "ev_pid", "ev_old", "ev_new", "re_obj", "re_rrc", "re_old", "re_new", "mo_off", "mr_obj"):
        assert np.array_equal(ta[k], tb[k]), (tag, k)


def test_random_windows_7x16(gpu_available):
    """300 objects: slots past one 256-slot property tile and four 64-slot record tiles.  Every call
    kind mixed, lists of one call and of more than 64, the objects in a tile's last slots among the
    touched.  The twin world has no links: handed the model's final value of every property an event
    named as a direct Set, its frames are the linked world's, bit for bit (a link's event is a
    standalone queued Set's)"""
    n = 300
    h = LHand(n, 7, 16, 7, COLS16, 41)
    twin = LHand(n, 7, 16, 7, COLS16, 41, link=False)
    try:
        rng = np.random.default_rng(9)
        edge = [0, 1, 2, 63, 64, 127, 255, 256, 299]
        n_ev = 0
        for w in range(4):
            touched = sorted(set(edge) | set(int(x) for x in rng.choice(n, 60, replace=False)))
            _random_window(h, rng, touched, twin=twin)
            if w == 0:
                h.call(5, ("set", 0, 3, 77))                         # a list of one call
                twin.call(5, ("set", 0, 3, 77), model=False)
                for k in range(70):                                  # a list longer than a wave
                    for hh, md in ((h, True), (twin, False)):
                        hh.call(2, ("set", k % 7, k % 16, k * 3 - 100), model=md)
                        hh.call(255, ("swap", k % 7, (k * 5) % 7), model=md)
            # the twin: the window's hits as direct Sets of the final values (every (object, pid) the
            # model set at least once; a Set back to the frame-start value raises nothing there either)
            for o in range(n):
                for pid in sorted(h.rec[o].start):
                    twin.m.set_props([twin.gh[o]], [twin.gd[o]], [pid], [u64(h.rec[o].props[pid])])
            ta, want = h.check_frame(f"window {w}")
            tb = twin.frame()
            _same_frame(ta, tb, f"window {w}")
            n_ev += sum(len(v) for v in want.values())
        assert n_ev > 300, n_ev
    finally:
        h.m.close()
        twin.m.close()


@pytest.mark.parametrize("rows_l", [64, 1])
def test_64x3(gpu_available, rows_l):
    """a 64-row record summed over all its rows (bit 63 of the mask counts), and one summed over
    row 0 alone"""
    n = 130
    h = LHand(n, 64, 3, rows_l, [PID["MAXHP"], -1, PID["ATK_VALUE"]], 5)
    try:
        rng = np.random.default_rng(rows_l)
        for w in range(2):
            _random_window(h, rng, sorted(set([0, 1, 2, 63, 64, 129]) | set(int(x) for x in rng.choice(n, 40, replace=False))),
                           lo=2, hi=12)
            h.call(2, ("set", 63, 0, (1 << 32) + 5))
            h.call(2, ("swap", 63, 2))
            h.call(2, ("set", 0, 0, -(1 << 31)))
            h.check_frame(f"window {w}")
    finally:
        h.m.close()


def test_reads_before_the_frame(gpu_available):
    """get_props, query_objects and snapshot_objects on linked properties with calls queued"""
    n = 300
    h = LHand(n, 7, 16, 7, COLS16, 43)
    try:
        rng = np.random.default_rng(3)
        touched = sorted(set([0, 1, 2, 255, 256, 299]) | set(int(x) for x in rng.choice(n, 80, replace=False)))
        _random_window(h, rng, touched)
        for o in touched[:20]:                  # values a query can meet
            h.call(o, ("add", 0, [4] + [0] * 15))
            h.call(o, ("set", 0, 1, 6))
        objs = np.repeat(np.arange(n), len(h.pids))
        pids = np.tile(np.array(h.pids, np.int32), n)
        got = h.m.get_props(h.gh[objs], h.gd[objs], pids).view(np.int64)
        want = [h.rec[o].props[p] for o, p in zip(objs.tolist(), pids.tolist())]
        assert got.tolist() == want
        # queries: players / others of the scene whose linked property equals a value, in (group, NFGUID) order
        qs, exp = [], []
        for pid, who in ((PID["MAXHP"], kernel.Q_PLAYERS), (PID["MAXHP"], kernel.Q_OTHERS), (PID["ATK_VALUE"], kernel.Q_PLAYERS)):
            vals = [h.rec[o].props[pid] for o in touched[:20]]
            v = max(set(vals), key=vals.count)
            qs.append(kernel.query(1, who=who, pid=pid, value=v))
            hit = [o for o in range(n) if (h.cls[o] == 1) == (who == kernel.Q_PLAYERS) and h.rec[o].props[pid] == v]
            exp.append(sorted(hit, key=lambda o: (h.group[o], h.gd[o])))
            assert any(o in touched for o in hit)
        got = h.m.query_objects(qs)
        assert [g.tolist() for g in got] == exp
        # snapshots (private view): the linked properties' entries
        sel = touched[:30] + [o for o in range(n) if o not in touched][:10]
        st = {}
        sn = h.m.snapshot_objects(h.gh[sel], h.gd[sel], np.full(len(sel), kernel.VIEW_PRIVATE, np.uint8), stats=st)
        for i, o in enumerate(sel):
            a, k = int(sn["p_first"][i]), int(sn["p_count"][i])
            ent = {int(p): rlm.s64(int(b)) for p, b in zip(sn["p_pid"][a:a + k], sn["p_bits"][a:a + k])}
            wantp = {p: h.rec[o].props[p] for p in h.pids
                     if h.rec[o].props[p] != 0 and (int(h.flags[h.cls[o]][p]) & PRIVATE)}
            assert {p: v for p, v in ent.items() if p in h.pids} == wantp, o
        h.check_frame("after the reads")
    finally:
        h.m.close()


HPREGEN_KIND = {workload.KID["HPRegen"]: [(workload.OP_IADD_CLAMP, workload.A_PROP | workload.HI_PROP, PID["HP"], 0,
                                           PID["HPREGEN"], 0, PID["MAXHP"])]}


@pytest.mark.parametrize("path", ["jit", "library", "touch"])
def test_program_clamps_to_a_linked_maxhp(gpu_available, monkeypatch, path):
    """HPRegen: HP = min(HP + HPREGEN, MAXHP) with MAXHP and HPREGEN both linked: the program sees the
    window's link values in the frame that applies them, on the hipRTC k_tick, the library's and
    k_tick_touch"""
    if path == "library":
        monkeypatch.setenv("NFGPU_JIT", "0")
    if path == "touch":
        monkeypatch.setenv("NFGPU_ABLATE", "8")
    n = 300
    col_pid = [PID["MAXHP"], PID["HPREGEN"], -1]
    h = LHand(n, 7, 3, 7, col_pid, 47, kinds=HPREGEN_KIND,
              before_commit=lambda hh: hh.m.load_prop(PID["HP"], np.full(n, 10, np.int64)))
    try:
        on, msg = h.m.jit_status()
        assert path == "touch" or bool(on) == (path == "jit"), msg
        kind = workload.KID["HPRegen"]
        h.m.add_schedules(h.gh, h.gd, np.full(n, kind, np.int32), np.full(n, 0.05, np.float32), np.full(n, -1, np.int32),
                          np.full(n, T0, np.int64))
        h.frame()                               # (the schedules exist from the end of this frame on)
        rng = np.random.default_rng(1)
        hp = np.full(n, 10, np.int64)
        for w in range(3):
            touched = sorted(set([0, 255, 256, 299]) | set(int(x) for x in rng.choice(n, 100, replace=False)))
            for o in touched:
                h.call(o, ("add", int(rng.integers(0, 7)), [int(rng.integers(0, 40)), int(rng.integers(0, 9)), 0]))
                h.call(o, ("set", int(rng.integers(0, 7)), 1, int(rng.integers(0, 9))))
            want = h.want_events()
            h.t += 100
            h.m.Execute(T0 + h.t)
            t = h.m.read_tick()
            fired = set(int(x) for x in t["fi_obj"])
            assert len(fired) == n, "every heartbeat fires every frame"
            maxhp = np.array([h.rec[o].props[PID["MAXHP"]] for o in range(n)])
            regen = np.array([h.rec[o].props[PID["HPREGEN"]] for o in range(n)])
            new_hp = np.minimum(np.maximum(hp + regen, 0), maxhp)       # IADD_CLAMP: clamp(hp + a, lo = 0, hi = MAXHP)
            for o in range(n):
                ev = [(PID["HP"], int(hp[o]), int(new_hp[o]))] if new_hp[o] != hp[o] else []
                ev = sorted(ev + want.get(o, []))
                got = [(int(t["ev_pid"][i]), rlm.s64(int(t["ev_old"][i])), rlm.s64(int(t["ev_new"][i])))
                       for i in np.nonzero(t["ev_obj"] == o)[0]]
                assert got == ev, (w, o)
            assert h.m.read_prop(PID["HP"]).tolist() == new_hp.tolist()
            hp = new_hp
            h.check_state(f"window {w}")
        assert (hp != 10).sum() > 100
    finally:
        h.m.close()


def test_execute_calls_applies_links(gpu_available):
    n = 300
    h = LHand(n, 7, 16, 7, COLS16, 53)
    try:
        rng = np.random.default_rng(2)
        for w in range(2):
            _random_window(h, rng, sorted(set([255, 256]) | set(int(x) for x in rng.choice(n, 30, replace=False))))
            _, want = h.check_frame(f"calls-only {w}", calls_only=True)
            assert want
    finally:
        h.m.close()


def test_links_without_calls_change_nothing(gpu_available):
    """links defined, no call on the linked record: frames bit-identical to the same world without
    links — record calls on the other record, direct Sets of unlinked properties, heartbeats"""
    n = 300
    col_pid = [PID["MAXHP"], PID["HPREGEN"], -1]
    worlds = [LHand(n, 7, 3, 7, col_pid, 59, link=lk, kinds=HPREGEN_KIND) for lk in (True, False)]
    try:
        frames = []
        for h in worlds:
            rng = np.random.default_rng(4)
            kind = workload.KID["HPRegen"]
            h.m.add_schedules(h.gh, h.gd, np.full(n, kind, np.int32), np.full(n, 0.05, np.float32),
                              np.full(n, -1, np.int32), np.full(n, T0, np.int64))
            h.frame()                           # (the schedules exist from the end of this frame on)
            out = []
            for w in range(3):
                for o in rng.choice(n, 50, replace=False):
                    o = int(o)
                    h.call(o, ("set", int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 5))), rec=1)
                    h.call(o, ("add", -1, None), rec=1)
                    h.m.set_props([h.gh[o]], [h.gd[o]], [PID["Gold"]], [int(rng.integers(0, 9))])
                t = h.frame()
                out.append(t)
                assert len(t["ev_obj"]) and len(t["re_obj"]) and len(t["fi_obj"])
            frames.append(out)
        for ta, tb in zip(*frames):
            _same_frame(ta, tb, "no calls on the linked record")
            for k in ("fi_obj", "fi_kind", "fi_rem"):
                assert np.array_equal(ta[k], tb[k])
        for p in range(N_INT):
            assert np.array_equal(worlds[0].m.read_prop(p), worlds[1].m.read_prop(p)), p
    finally:
        for h in worlds:
            h.m.close()


def _bare(n_rec=2):
    m = kernel.NFKernelModule(8, n_class=2, n_rec=n_rec)
    for c in range(2):
        m.set_prop_flags(c, workload._prop_flags()[c])
    m.define_record(0, 7, 4, [0, 0, 1, 0], [PRIVATE, PRIVATE])       # column 2 is f64
    if n_rec > 1:
        m.define_record(1, 4, 2, [0, 0], [PRIVATE, PRIVATE])
    return m


def _refused(fn, code=-1):
    with pytest.raises(NFKError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_link_time_refusals(gpu_available):
    m = _bare()
    try:
        ok = [PID["MAXHP"], PID["ATK_VALUE"], -1, -1]
        _refused(lambda: m.link_record(2, 7, ok))                                    # a bad record
        _refused(lambda: m.link_record(-1, 7, ok))
        _refused(lambda: m.link_record(0, 0, ok))                                    # rows outside [1, rows]
        _refused(lambda: m.link_record(0, 8, ok))
        _refused(lambda: m.link_record(0, 7, [PID["MAXHP"], -1, PID["ATK_VALUE"], -1]))   # an f64 column
        _refused(lambda: m.link_record(0, 7, [PID["X"], -1, -1, -1]))                # a float property
        _refused(lambda: m.link_record(0, 7, [N_INT + N_FLT, -1, -1, -1]))           # no property
        _refused(lambda: m.link_record(0, 7, [-2, -1, -1, -1]))
        _refused(lambda: m.link_record(0, 7, [PID["MAXHP"], PID["MAXHP"], -1, -1]))  # twice in one record
        m.link_record(0, 7, ok)
        _refused(lambda: m.link_record(1, 4, [PID["ATK_VALUE"], -1]))                # from another record
        m.link_record(0, 7, ok)                                                      # (the same link again: its own pids)
        m.link_record(0, 7, None)                                                    # unlink
        m.link_record(1, 4, [PID["ATK_VALUE"], -1])
        assert m.lib.nfk_link_record(m.h, 0, 7, kernel._p(np.array([PID["MAXHP"], -1, -1, -1], np.int32)), 1) == -1   # a mode that is not SUM32
        # nfk_set_scene_props' properties, in both orders
        m.set_scene_props(PID["SceneID"], PID["GroupID"], PID["X"], PID["Y"], PID["Z"])
        _refused(lambda: m.link_record(0, 7, [PID["SceneID"], -1, -1, -1]))
        _refused(lambda: m.link_record(0, 7, [PID["GroupID"], -1, -1, -1]))
        m.set_scene_props(-1, -1, -1, -1, -1)
        m.link_record(0, 7, [PID["Camp"], -1, -1, -1])
        _refused(lambda: m.set_scene_props(PID["Camp"], PID["GroupID"], -1, -1, -1))
        _refused(lambda: m.set_scene_props(PID["SceneID"], PID["Camp"], -1, -1, -1))
        gh, gd = np.full(8, 7, np.int64), np.arange(1, 9, dtype=np.int64)
        m.create_objects(gh, gd, np.ones(8, np.int32), np.ones(8, np.int32), np.zeros(8, np.uint8), np.zeros(8, np.uint8))
        m.commit()
        _refused(lambda: m.link_record(0, 7, ok), code=-3)                           # NFK_ERR_STATE after commit
    finally:
        m.close()


@pytest.mark.parametrize("case", ["program writes a linked property", "record op on a linked column",
                                  "program reads a linked property"])
def test_commit_time_refusals(gpu_available, case):
    m = _bare(1)
    try:
        m.link_record(0, 7, [PID["MAXHP"], PID["ATK_VALUE"], -1, -1])
        if case == "program writes a linked property":
            ops = [(workload.OP_ISET, 0, PID["MAXHP"], 0, 5, 0, 0)]
        elif case == "record op on a linked column":
            ops = [(workload.OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, 1, 0, 100)]
        else:   # operands, NFK_HI_PROP, a guard on a linked property, a cell guard on a linked cell: legal;
            # a record op on an UNLINKED column of the linked record too
            ops = [(workload.OP_IADD_CLAMP, workload.A_PROP | workload.HI_PROP | workload.GUARD, PID["HP"],
                    workload.guard(PID["ATK_VALUE"], workload.GUARD_GT0), PID["ATK_VALUE"], 0, PID["MAXHP"]),
                   (workload.OP_ISET, workload.GUARD | workload.GUARD_CELL, PID["MP"],
                    workload.guard_cell(0, 1, 0, workload.GUARD_GT0), 1, 0, 0),
                   (workload.OP_RIADD_CLAMP, 0, (0 << 8) | 3, 0, 1, 0, 100)]
        m.define_kind(0, np.array(ops, workload.OP_DTYPE))
        gh, gd = np.full(8, 7, np.int64), np.arange(1, 9, dtype=np.int64)
        m.create_objects(gh, gd, np.ones(8, np.int32), np.ones(8, np.int32), np.zeros(8, np.uint8), np.zeros(8, np.uint8))
        if case == "program reads a linked property":
            m.commit()
        else:
            assert "linked" in _refused(m.commit)
    finally:
        m.close()


def test_direct_sets_of_a_linked_property_are_refused(gpu_available):
    """the one difference from the reference: a queued direct Set of a linked property is
    NFK_ERR_ARG and its batch queues nothing; spawn values keep working"""
    n = 20
    h = LHand(n, 7, 16, 7, COLS16, 61)
    try:
        m = h.m
        gold, maxhp, scene = PID["Gold"], PID["MAXHP"], PID["SceneID"]
        _refused(lambda: m.set_props(h.gh[:2], h.gd[:2], [scene, maxhp], [5, 6]))
        _refused(lambda: m.set_props_obj([0, 1], [scene, maxhp], [5, 6]))
        t = h.frame()
        assert len(t["ev_obj"]) == 0, "a refused batch queued nothing"
        m.set_props(h.gh[:1], h.gd[:1], [scene], [5])
        t = h.frame()
        assert t["ev_obj"].tolist() == [0] and t["ev_pid"].tolist() == [scene]
        # a spawned object's linked properties take the values it is spawned with, and its link works
        props = np.zeros((1, N_INT + N_FLT), np.uint64)
        props[0, maxhp] = 123
        m.spawn_objects([7], [1000], [1], [1], [1], [1], props)
        m.record_rows([7], [1000], [0], [1], [0], [[9] + [0] * 15])
        assert int(m.get_props([7], [1000], [maxhp]).view(np.int64)[0]) == 9
        m.Execute(T0 + 10_000)
        t = m.read_tick()
        ev = [(int(p), int(a), int(b)) for p, a, b in zip(t["ev_pid"], t["ev_old"], t["ev_new"])]
        assert (maxhp, 123, 9) in ev, ev
        assert int(m.get_props([7], [1000], [maxhp]).view(np.int64)[0]) == 9
    finally:
        h.m.close()


def test_cpp_plugin(gpu_available, tmp_path):
    """NFGPUKernelModule::LinkRecordColumns over the golden script, line for line against the answers
    recorded from the compiled NFCPropertyModule: after every call GetPropertyInt of the object's
    linked properties (the window's queued calls replayed), the calls' return values where the plugin
    answers what the reference does, SetPropertyInt refused on a linked name, and per frame the
    property events the common callback receives against the model's window rule"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "record_link.json")) as f:
        g = json.load(f)
    script, answers = list(g["script"]), [list(a) for a in g["answers"]]
    tags = next(ln for ln in script if ln.startswith("TAGS ")).split()[1:]
    # one more line behind the golden's last frame: a direct Set of a linked name (refused, nothing queued)
    last = next(k for k in range(len(script) - 1, -1, -1) if script[k].split()[0] not in ("X",))
    o_last = int(script[last].split()[1])
    script.append(f"SP {o_last} MAXHP 12345")
    answers.append([0, answers[-1][1]])
    script.append("X")
    sp = tmp_path / "script.txt"
    sp.write_text("\n".join(script) + "\n")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "_bin", "record_link_plugin"), str(sp)], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[0] == "R refused", "a record with an object column was linked"
    got, got_ev = [], {}
    for ln in run.stdout.splitlines():
        if ln.startswith("A "):
            head, lst = ln.split(":")
            f = head.split()
            assert int(f[1]) == len(got), ln
            got.append([int(f[2]), [int(x) for x in lst.split()]])
        elif ln.startswith("P "):
            f = ln.split()
            got_ev.setdefault((int(f[1]), int(f[2])), []).append((f[3], int(f[4]), int(f[5])))
    calls = [ln for ln in script if ln.split()[0] not in ("SHAPE", "TAGS", "BASE", "OBJ", "X")]
    assert len(got) == len(answers) == len(calls)
    n_ret = 0
    for k, (a, b) in enumerate(zip(got, answers)):
        assert a[1] == b[1], (k, calls[k], a, b)
        # (SetRecordInt answers true once queued where the reference answers false for an unchanged value)
        if calls[k].split()[0] in ("AR", "RM", "CL", "SW", "SP", "LV"):
            assert a[0] == b[0], (k, calls[k], a, b)
            n_ret += 1
    assert n_ret > 100
    # the frames' property events: the model's window rule over the golden script (the model replays the
    # golden's answers: tests/test_record_link.py)
    want_ev, win = {}, [0]
    objs = {}

    def watch(k, f, rec):
        if k is None:
            for o, r in objs.items():
                ev = r.frame_events()
                if ev:
                    want_ev[(win[0], o)] = [(tags[p], a, b) for p, a, b in ev]
            win[0] += 1
        else:
            objs[int(f[1])] = rec
    rlm.replay([ln for ln in script if not ln.startswith("SP ")], watch)
    assert sorted(got_ev) == sorted(want_ev)
    for key in want_ev:
        assert got_ev[key] == want_ev[key], key
    assert sum(len(v) for v in want_ev.values()) > 60
