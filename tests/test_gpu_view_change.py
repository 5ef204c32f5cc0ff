"""GPU: nfk_view_changes against tests/view_change_model.py — the window's log, every entry's visits and
both lists of every visit compared in order — over random windows of every kind of membership call on
a world with a three-tile group, small groups, populated group 0s, an emptied group and groups that
never existed; the frames beside it bit-identical to a twin world that never asks; a batch of more
than 1024 tiles; a group past the stint cap (answered on the host); and the plugin's
AddObjectEnterCallBack / AddObjectLeaveCallBack over the golden script."""
import json
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import kernel, workload
from tests import view_change_model as vcm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = workload.PID
N_PW = workload.N_INT + workload.N_FLT


def layout(n_obj, cells, seed):
    """a workload whose objects sit in the given [(scene, group, members, players)] cells"""
    assert sum(c[2] for c in cells) == n_obj
    w = dict(workload.make_world(n_obj=n_obj, n_scenes=1, groups_per_scene=4, players_per_group=2, n_ticks=8,
                                 seed=seed, host_ops=False, ext_frac=0.0))
    scene, group, pl = (np.zeros(n_obj, np.int32) for _ in range(3))
    at = 0
    for s, g, n, p in cells:
        scene[at:at + n], group[at:at + n] = s, g
        pl[at:at + p] = 1
        at += n
    perm = np.random.default_rng(seed).permutation(n_obj)   # creation order is not layout order
    w["scene"], w["group"] = scene[perm], group[perm]
    w["is_player"] = pl[perm].astype(np.uint8)
    w["cls"] = np.where(w["is_player"] == 1, workload.CLS_PLAYER, workload.CLS_NPC).astype(np.uint8)
    w["init_i"] = w["init_i"].copy()
    w["init_i"][PID["SceneID"]], w["init_i"][PID["GroupID"]] = w["scene"], w["group"]
    return w


class Twins:
    """the same calls on world A (asked for its view changes), world B (never asked) and the model"""

    def __init__(self, w, room):
        import torch
        self.torch = torch
        self.w = w
        n = len(w["guid_head"])
        self.ms = [kernel.world_from_workload(w, capacity=n + room) for _ in range(2)]
        self.a = self.ms[0]
        self.model = vcm.Model(w["guid_head"], w["guid_data"], w["scene"], w["group"], w["is_player"])
        self.next_guid = 1
        self.cls = [int(c) for c in w["cls"]]

    def close(self):
        for m in self.ms:
            m.close()

    def guid(self, o):
        return self.model.gh[o], self.model.gd[o]

    def switch(self, o, s, g):
        for m in self.ms:
            m.SwitchScene(self.guid(o), s, g, 1.5, 2.5, 3.5)
        self.model.switch(o, s, g)

    def destroy(self, objs):
        gh, gd = zip(*[self.guid(o) for o in objs])
        for m in self.ms:
            m.destroy_objects(gh, gd)
        for o in objs:
            self.model.destroy(o)

    def spawn(self, cells, players):
        n = len(cells)
        gh, gd = np.full(n, 11, np.int64), np.arange(self.next_guid, self.next_guid + n, dtype=np.int64)
        self.next_guid += n
        cls = [workload.CLS_PLAYER if p else workload.CLS_NPC for p in players]
        for m in self.ms:
            m.spawn_objects(gh, gd, [c[0] for c in cells], [c[1] for c in cells], cls, players,
                            np.zeros((n, N_PW), np.uint64))
        self.cls += cls
        return [self.model.create(gh[i], gd[i], cells[i][0], cells[i][1], players[i]) for i in range(n)]

    def migrate(self, objs, cells):
        """export, then import under the same NFGUIDs into `cells` (new object indices)"""
        gh, gd = zip(*[self.guid(o) for o in objs])
        pl = [self.model.player[o] for o in objs]
        cls = [self.cls[o] for o in objs]
        for m in self.ms:
            rows = self.torch.zeros((len(objs), m.row_words()), dtype=self.torch.int64, device="cuda")
            m.export_objects(gh, gd, rows.data_ptr())
            m.import_objects(gh, gd, [c[0] for c in cells], [c[1] for c in cells], cls, pl, rows.data_ptr())
            m.synchronize()
        for o in objs:
            self.model.export(o)
        self.cls += cls
        return [self.model.create(gh[i], gd[i], cells[i][0], cells[i][1], pl[i]) for i in range(len(objs))]

    def check(self, tag, n_host=0):
        got = self.a.view_changes()
        vcm.compare(got, self.model, tag)
        if n_host == 0:
            assert got["n_host"] == 0, tag
        return got

    def frame(self, t):
        """execute the window on both worlds: their events and recipient lists are bit-identical"""
        outs = []
        for m in self.ms:
            kernel.run_workload(m, self.w, t)
            outs.append(m.read_tick())
        for k, v in outs[0].items():
            if k == "summary":
                continue
            assert v.dtype == outs[1][k].dtype and np.array_equal(v, outs[1][k]), f"frame {t}: {k} differs"
        assert outs[0]["summary"]["n_msgs"] == outs[1]["summary"]["n_msgs"]
        self.model.begin_window()
        return outs[0]


BIG = (1, 1)        # ~700 members, 60 players: three tiles
EMPTIED = (2, 5)    # emptied by the first window
MAIN_CELLS = ([(1, 1, 700, 60), (1, 0, 60, 9), (2, 0, 50, 7), (3, 0, 45, 5), (2, 5, 12, 3), (2, 6, 1, 1),
               (1, 2, 1, 0), (1, 3, 40, 6), (1, 4, 17, 2), (2, 1, 33, 4), (2, 2, 5, 5), (2, 3, 26, 3),
               (3, 1, 40, 0), (3, 2, 9, 1), (3, 3, 2, 2), (1, 5, 100, 10), (2, 7, 121, 14), (3, 4, 39, 8),
               (3, 5, 120, 12), (2, 8, 80, 0)])


@pytest.fixture(scope="module")
def main_world(gpu_available):
    n = sum(c[2] for c in MAIN_CELLS)
    assert 1400 <= n <= 1600
    tw = Twins(layout(n, MAIN_CELLS, 31), room=400)
    yield tw
    tw.close()


def test_random_windows(main_world):
    """6 windows of about 40 calls: every kind of call, NPCs switch too, movers drawn with repetition"""
    tw = main_world
    md = tw.model
    rng = np.random.default_rng(77)
    # window 0 empties one group (its segment is dropped by the re-layout: the group stays known)
    for o in sorted(md.members[EMPTIED]):
        tw.switch(o, 2, 6)
    got = tw.check("emptying window")
    assert tw.a.view_changes()["obj"].tolist() == got["obj"].tolist()
    tw.frame(0)
    assert not md.members[EMPTIED]
    never = 90
    seen_kinds, seen_why = set(), set()
    shapes = {"double": 0, "return": 0, "create_destroy": 0}
    for win in range(1, 7):
        alive = [o for o in range(len(md.gh)) if md.alive[o]]
        big = sorted(md.members[BIG])
        pool = [int(x) for x in rng.choice(big, 4)] + [int(x) for x in rng.choice(alive, 8)]
        assert any(not md.player[o] for o in pool)
        targets = [BIG, BIG, (1, 0), (2, 0), (3, 0), EMPTIED, (1, 2), (2, 2), (3, 3), (1, 4), (3, never + win),
                   (2, never + win)]
        pick = lambda: targets[int(rng.integers(len(targets)))]
        start = {o: (md.scene[o], md.group[o]) for o in pool}
        moved, born = set(), []
        # every kind of call occurs: a migration (export + import), a spawn, a destroy, then the draw
        fresh = [o for o in alive if o not in pool][:2]
        born += tw.migrate(fresh, [pick(), pick()])
        born += tw.spawn([pick(), BIG, (2, 0)], [1, 0, 1])
        tw.destroy([born[-1]])
        shapes["create_destroy"] += 1
        n_calls = 7
        while n_calls < 40:
            r = rng.random()
            cand = [o for o in pool + born if md.alive[o]]
            if r < 0.75 and cand:
                o = cand[int(rng.integers(len(cand)))]
                s, g = pick() if rng.random() < 0.8 or o not in start else start[o]
                if (s, g) == (md.scene[o], md.group[o]):
                    tw.switch(o, s, g)   # (neither scene nor group changes: nothing is logged)
                    continue
                if o in moved:
                    shapes["double"] += 1
                    if o in start and (s, g) == start[o]:
                        shapes["return"] += 1
                moved.add(o)
                tw.switch(o, s, g)
            elif r < 0.87:
                k = int(rng.integers(1, 4))
                born += tw.spawn([pick() for _ in range(k)], [int(rng.random() < 0.5) for _ in range(k)])
                n_calls += k - 1
            elif len(cand) > 4:
                o = cand[int(rng.integers(len(cand)))]
                if o in born:
                    shapes["create_destroy"] += 1
                tw.destroy([o])
            else:
                continue
            n_calls += 1
        got = tw.check(f"window {win}")
        seen_kinds |= set(got["log"][:, 1].tolist())
        seen_why |= set(got["visit"][:, 0].tolist())
        assert set(got["log"][:, 1].tolist()) == {0, 1, 2, 3}, "every kind of call in every window"
        assert len(md.log) >= 35
        again = tw.a.view_changes()   # twice in a window: the same answer
        for k in ("log", "call_visit", "visit", "visit_off", "obj"):
            assert np.array_equal(again[k], got[k]), k
        tw.frame(win)
    assert seen_why == {0, 1, 2, 3, 4}
    assert all(v > 0 for v in shapes.values()), shapes


def test_more_calls_between_two_answers(main_world):
    """the second call of a window answers the first call's entries the same, plus what was queued since"""
    tw = main_world
    md = tw.model
    objs = sorted(md.members[(1, 3)])[:3]
    tw.switch(objs[0], 1, 4)
    first = tw.check("first")
    tw.switch(objs[1], 1, 4)
    tw.switch(objs[0], 1, 3)
    both = tw.check("second")
    n = int(first["visit_off"][-1])
    assert both["log"][:1].tolist() == first["log"].tolist()
    assert both["obj"][:n].tolist() == first["obj"].tolist()
    tw.frame(7)
    assert tw.a.view_changes()["log"].shape == (0, 6)   # the log is cleared where the window is applied


@pytest.fixture(scope="module")
def wide_world(gpu_available):
    # 1,200 players in 600 groups of two, and a few NPCs beside them
    cells = [(1, g, 2, 2) for g in range(1, 601)] + [(1, 0, 40, 0), (1, 700, 60, 0)]
    tw = Twins(layout(1300, cells, 41), room=16)
    yield tw
    tw.close()


def test_wide_batch(wide_world):
    """1,200 players each leave a small group for the next one in one window: more than 1024 tiles, so the
    scan's lanes take more than one count each"""
    tw = wide_world
    md = tw.model
    movers = [o for o in range(1300) if md.player[o]]
    assert len(movers) == 1200
    for o in movers:
        tw.switch(o, 1, md.group[o] % 600 + 1)
    got = tw.check("wide")
    assert got["n_tiles"] > 1024 and len(got["visit"]) == 2400
    tw.frame(0)


def test_past_the_stint_cap(wide_world):
    """more than NFK_VC_STINT_CAP objects enter one group in a window: its later visits are answered on
    the host, with the same lists"""
    tw = wide_world
    md = tw.model
    movers = [o for o in range(1300) if md.player[o] and md.group[o] != 7][:kernel.VC_STINT_CAP + 40]
    for o in movers:
        tw.switch(o, 1, 7)
    tw.switch(movers[0], 1, 0)
    tw.switch(sorted(md.members[(1, 700)])[0], 1, 7)
    got = tw.check("past the cap", n_host=None)
    assert got["n_host"] > 0
    tw.frame(1)
    tw.switch(movers[1], 1, 9)   # the next window: under the cap again
    tw.check("after")
    tw.frame(2)


def test_before_commit(gpu_available):
    m = kernel.NFKernelModule(16)
    try:
        with pytest.raises(kernel.NFKError) as e:
            m.view_changes()
        assert e.value.code == -3   # NFK_ERR_STATE
    finally:
        m.close()


def test_plugin_replays_the_golden_script(gpu_available, tmp_path):
    """tests/cpp/view_change_plugin.cpp: the golden script through AddObjectEnterCallBack /
    AddObjectLeaveCallBack prints the reference's OnObjectListEnter / OnObjectListLeave lines"""
    exe = os.path.join(ROOT, "tests", "cpp", "_bin", "view_change_plugin")
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "view_change.json")))
    script = tmp_path / "script.txt"
    script.write_text("\n".join(want["script"]) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want["lines"])
    for i, (g, w) in enumerate(zip(got, want["lines"])):
        assert g == w, f"call {i}"
