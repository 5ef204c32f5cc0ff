"""nfk_view_changes restated in Python: the window's membership log, each entry's visits (the groups
NFCSceneAOIModule::OnGroupEvent / OnSceneEvent / OnClassCommonEvent read, AOI:292-529, in the
reference's order) and, per visit, the group's players and its other objects in NFGUID order as the
group stood at the visit's call; and the OnObjectListEnter / OnObjectListLeave calls the reference
composes from those lists (`compose`).

Membership is kept eagerly: a call changes the model's groups at once and records its visits' lists as
it is made, which is what the reference does.  The device derives the same lists afterwards from the
frame-start layout and the log."""
import numpy as np

VC_SWITCH, VC_DESTROY, VC_CREATE, VC_EXPORT = 0, 1, 2, 3
GROUP_LEAVE, GROUP_ENTER, SCENE_LEAVE, SCENE_ENTER, WHY_DESTROY = 0, 1, 2, 3, 4


def visits_of(kind, s0, g0, s1, g1):
    """entry -> [(why, scene, group)] in the reference's order"""
    v = []
    if kind == VC_SWITCH:
        if g0 > 0:
            v.append((GROUP_LEAVE, s0, g0))          # AOI:361-387 (GroupID old -> 0 or -> g1)
        if s0 != s1:
            v.append((SCENE_LEAVE, s0, 0))           # AOI:473-526 (the SceneID write, KM:935)
            v.append((SCENE_ENTER, s1, 0))
        if g1 > 0:
            v.append((GROUP_ENTER, s1, g1))          # AOI:396-455
    elif kind == VC_DESTROY:
        if s0 > 0:
            v.append((WHY_DESTROY, s0, g0))          # AOI:294-327
    elif kind == VC_CREATE:
        if s1 != 0:
            v.append((SCENE_ENTER, s1, 0))           # KM:248 (SceneID), then KM:249 (GroupID)
        if g1 > 0:
            v.append((GROUP_ENTER, s1, g1))
    else:
        if g0 > 0:
            v.append((GROUP_LEAVE, s0, g0))
        v.append((SCENE_LEAVE, s0, 0))
    return v


class Model:
    def __init__(self, guid_head, guid_data, scene, group, is_player):
        self.gh = [int(x) for x in guid_head]
        self.gd = [int(x) for x in guid_data]
        self.scene = [int(x) for x in scene]
        self.group = [int(x) for x in group]
        self.player = [bool(x) for x in is_player]
        self.alive = [True] * len(self.gh)
        self.members = {}
        for o in range(len(self.gh)):
            self.members.setdefault((self.scene[o], self.group[o]), set()).add(o)
        self.begin_window()

    def begin_window(self):
        self.log, self.call_visit, self.visit, self.lists = [], [0], [], []

    def _lists(self, s, g, skip):
        m = sorted((o for o in self.members.get((s, g), ()) if o != skip), key=lambda o: (self.gh[o], self.gd[o]))
        return [o for o in m if self.player[o]], [o for o in m if not self.player[o]]

    def _entry(self, o, kind, s0, g0, s1, g1):
        self.log.append((o, kind, s0, g0, s1, g1))
        for why, s, g in visits_of(kind, s0, g0, s1, g1):
            self.visit.append((why, s, g))
            self.lists.append(self._lists(s, g, o))
        self.call_visit.append(len(self.visit))

    def switch(self, o, s1, g1):
        s0, g0 = self.scene[o], self.group[o]
        if (s0, g0) == (s1, g1):
            return
        self.members[(s0, g0)].discard(o)            # out of the old group at its own instant (KM:929)
        self._entry(o, VC_SWITCH, s0, g0, s1, g1)
        self.members.setdefault((s1, g1), set()).add(o)   # (KM:945)
        self.scene[o], self.group[o] = s1, g1

    def _leave(self, o, kind):
        s0, g0 = self.scene[o], self.group[o]
        self.members[(s0, g0)].discard(o)            # (KM:291 precedes the COE_DESTROY event's reads)
        self.alive[o] = False
        self._entry(o, kind, s0, g0, 0, 0)

    def destroy(self, o):
        self._leave(o, VC_DESTROY)

    def export(self, o):
        self._leave(o, VC_EXPORT)

    def create(self, gh, gd, s, g, is_player):
        o = len(self.gh)
        self.gh.append(int(gh))
        self.gd.append(int(gd))
        self.scene.append(int(s))
        self.group.append(int(g))
        self.player.append(bool(is_player))
        self.alive.append(True)
        self.members.setdefault((s, g), set()).add(o)     # in its group at its own instant (KM:146): skipped as self
        self._entry(o, VC_CREATE, 0, 0, s, g)
        return o


def compare(got, model, tag=""):
    """kernel.view_changes()'s dict against the model's window: the log, the visits and both lists of
    every visit, in order"""
    assert got["log"].tolist() == [list(e) for e in model.log], f"{tag}: log"
    assert got["call_visit"].tolist() == model.call_visit, f"{tag}: call_visit"
    assert got["visit"].tolist() == [list(v) for v in model.visit], f"{tag}: visits"
    off, obj = got["visit_off"], got["obj"]
    assert len(off) == 2 * len(model.visit) + 1
    for v, (pl, ot) in enumerate(model.lists):
        a, m, b = int(off[2 * v]), int(off[2 * v + 1]), int(off[2 * v + 2])
        assert obj[a:m].tolist() == pl, f"{tag}: visit {v} {model.visit[v]} players ({m - a} vs {len(pl)})"
        assert obj[m:b].tolist() == ot, f"{tag}: visit {v} {model.visit[v]} others ({b - m} vs {len(ot)})"
    assert obj.dtype == np.int32


# ---- the reference's calls (AOI:292-529) composed from an entry's lists ----
def compose(entry, lists, self_player):
    """[(\"E\" | \"L\", to, about)]: the OnObjectListEnter / OnObjectListLeave calls the reference makes
    for one log entry, from the (players, others) lists of its visits in order"""
    o, kind, s0, g0, s1, g1 = entry
    it = iter(lists)
    me, out = [o], []

    def group_leave(pl, ot):     # AOI:361-387: both calls only when the old group is not empty
        if pl or ot:
            out.append(("L", pl, me))
            out.append(("L", me, pl + ot))

    def group_enter(pl, ot):     # AOI:396-437
        if pl:
            out.append(("E", pl, me))
        if (pl or ot) and self_player:
            out.append(("E", me, pl + ot))

    def scene_event(old, new, self_in_new):   # AOI:506-513; AOI:508 tests the players WITH self
        out.append(("L", me, old[0] + old[1]))
        if new[0] or (self_in_new and self_player):
            out.append(("E", new[0], me))
        out.append(("E", me, new[0] + new[1]))

    if kind == VC_SWITCH:
        if g0 > 0:
            group_leave(*next(it))
        if s0 != s1:
            old = next(it)
            scene_event(old, next(it), False)
        if g1 > 0:
            group_enter(*next(it))
    elif kind == VC_DESTROY:
        if s0 > 0:
            out.append(("L", next(it)[0], me))      # AOI:326, even when nobody is told
    elif kind == VC_CREATE:
        if s1 != 0:
            scene_event(([], []), next(it), g1 == 0)   # (SceneID 0 -> s: scene 0 holds nobody)
        if g1 > 0:
            group_enter(*next(it))
        if self_player:
            out.append(("E", me, me))               # COE_CREATE_HASDATA (AOI:341)
    else:
        if g0 > 0:
            group_leave(*next(it))
        out.append(("L", me, sum(next(it), [])))
    return out


def window_lines(model):
    """the model's window as the printed lines of view_change_ref / view_change_plugin"""
    lines = []
    for i, e in enumerate(model.log):
        a, b = model.call_visit[i], model.call_visit[i + 1]
        for k, to, about in compose(e, model.lists[a:b], model.player[e[0]]):
            lines.append(k + "".join(f" {x}" for x in to) + " :" + "".join(f" {x}" for x in about))
    return lines


# ---- the golden script (tests/golden/view_change.json) ----
def script_guid(i):
    """object i's NFGUID: not in index order"""
    return 7, (i * 37) % 101 + 1


def golden_script():
    """SCENE s / GRP s g (the group exists from here on) / OBJ i P|N s g (before the first frame) / INIT,
    then windows of SW i s g / CR i P|N s g / DE i closed by X.  Only Players switch."""
    s = ["SCENE 1", "SCENE 2", "SCENE 3", "GRP 1 3", "GRP 2 2"]
    objs = [("P", 1, 1), ("P", 1, 2), ("P", 1, 1), ("N", 1, 1), ("N", 1, 2), ("P", 1, 0), ("P", 2, 0), ("N", 2, 0),
            ("P", 2, 1), ("P", 1, 3), ("N", 1, 0), ("P", 2, 2), ("N", 2, 1), ("P", 1, 2)]
    s += [f"OBJ {i} {c} {sc} {g}" for i, (c, sc, g) in enumerate(objs)]
    s += ["INIT"]
    # two objects swap groups, one switches twice, one returns to its frame-start group
    s += ["SW 0 1 2", "SW 1 1 1", "SW 2 1 2", "SW 2 1 3", "SW 13 1 1", "SW 13 1 2", "X"]
    # created then destroyed; a create into group 0; an NPC into a new group; a player alone leaves for
    # a group that never existed
    s += ["CR 14 P 1 1", "DE 14", "CR 15 N 1 2", "DE 15", "CR 16 P 2 0", "GRP 1 4", "CR 17 N 1 4", "SW 2 1 1",
          "GRP 1 5", "SW 9 1 5", "X"]
    # (the last window: a Player created where no player is, AOI:508's test on the list with self)
    # into an emptied group; group 0 on either side; cross-scene with g0 = 0 and g0 > 0; destroys
    s += ["SW 1 1 3", "SW 5 1 2", "SW 0 1 0", "SW 6 1 1", "SW 8 1 0", "SW 11 1 2", "DE 3", "DE 5", "CR 18 P 1 3",
          "SW 1 2 2", "X"]
    s += ["SW 6 2 0", "DE 12", "SW 8 2 1", "SW 16 2 1", "DE 9", "SW 18 1 5", "CR 19 P 3 0", "X", "X"]
    return s


def replay_script(script):
    """(lines per the model, the cases the script holds) — objects are script indices"""
    objs, cases, lines = [], set(), []
    model, known = None, set()
    win, born = {}, set()
    for ln in script:
        f = ln.split()
        if f[0] == "OBJ":
            assert int(f[1]) == len(objs)
            objs.append((f[2] == "P", int(f[3]), int(f[4])))
            known.add((int(f[3]), int(f[4])))
        elif f[0] == "INIT":
            g = [script_guid(i) for i in range(len(objs))]
            model = Model([x[0] for x in g], [x[1] for x in g], [o[1] for o in objs], [o[2] for o in objs],
                          [o[0] for o in objs])
            start = {}
        elif f[0] == "SW":
            o, s1, g1 = int(f[1]), int(f[2]), int(f[3])
            assert model.player[o], "only Players switch (KM:929 / 945 file every mover under the player lists)"
            s0, g0 = model.scene[o], model.group[o]
            start.setdefault(o, (s0, g0))
            there = model.members.get((s1, g1), set())
            cases.add("twice" if o in win else "once")
            if (s1, g1) == start[o] and o in win:
                cases.add("return")
            if (s1, g1) not in known:
                cases.add("never_existed")
            elif not there:
                cases.add("into_empty")
            if g0 == 0 or g1 == 0:
                cases.add("group0_from" if g0 == 0 else "group0_to")
            if s0 != s1:
                cases.add("cross_g0_zero" if g0 == 0 else "cross_g0_positive")
            if g0 > 0 and not (model.members[(s0, g0)] - {o}):
                cases.add("player_alone")
            for p, (ps0, pg0, ps1, pg1) in win.items():
                if p != o and (ps0, pg0) == (s1, g1) and (ps1, pg1) == (s0, g0):
                    cases.add("swap")
            win[o] = (s0, g0, s1, g1)
            known.add((s1, g1))
            model.switch(o, s1, g1)
        elif f[0] == "CR":
            o = model.create(*script_guid(int(f[1])), int(f[3]), int(f[4]), f[2] == "P")
            assert o == int(f[1])
            known.add((int(f[3]), int(f[4])))
            born.add(o)
        elif f[0] == "DE":
            if int(f[1]) in born:
                cases.add("create_destroy")
            model.destroy(int(f[1]))
        elif f[0] == "X":
            lines += window_lines(model)
            model.begin_window()
            win, start, born = {}, {}, set()
    return lines, cases


GOLDEN_CASES = {"swap", "twice", "return", "create_destroy", "into_empty", "never_existed", "group0_from",
                "group0_to", "cross_g0_zero", "cross_g0_positive", "player_alone"}
