"""GPU: membership, slot reuse and table growth over long heavy-churn runs (tests/churn_worlds.py): every
frame of every world bit for bit against the oracle at four slack settings, on the three k_tick paths,
with the NFGUID lookups on the device mirror, through the consumer's per-frame read; the state BETWEEN
frames (group lists, online counts, record finds, enter snapshots) against the models over the helper's
membership, with objects in slots others held; the arrivals' row buffer past its first 1024 rows; the
`churn` golden recorded from the compiled reference.

Every run prints a line `CHURN_STATS <world> slack=<s> n_full=<..> n_seg=<..> tiles=<min>-<max>`
(pytest -s shows them; profiles/churn_gpu_tests.txt keeps the ones observed)."""
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import kernel, nfio, workload
from noahgameframe_amd.kernel import Q_OTHERS, Q_PLAYERS, query
from tests import churn_worlds as cw
from tests import scene_query_model as sqm
from tests.parity import ROOT, compare_runs, run_gpu, run_oracle
from tests.record_find_model import Record
from tests.test_gpu_enter_snapshot import PRIV, PUB, Model
from tests.test_gpu_parity import PATHS, set_path
from tests.test_gpu_rank_in_tick import run_frames
from tests.test_gpu_scene_query import Driver

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
PID, N_INT, N_FLT = workload.PID, workload.N_INT, workload.N_FLT
FRAME_KEYS = ("ev_obj", "ev_pid", "ev_old", "ev_new", "re_obj", "re_rrc", "re_old", "re_new", "fi_obj", "fi_kind", "fi_rem")

_oracle = {}


def oracle(name):
    """the oracle's run of a named world, computed once and left unchanged"""
    if name not in _oracle:
        _oracle[name] = run_oracle(cw.world(name))
    return _oracle[name]


def run(w, slack_per_256=0):
    """tests.parity.run_gpu, and the world's membership_stats() and tile counts: (outputs, stats)"""
    m = kernel.world_from_workload(w, slack_per_256=slack_per_256)
    out, tiles = {}, []
    try:
        for t in range(int(w["cfg"][7])):
            r = kernel.run_workload(m, w, t)
            assert r["summary"]["device_error"] == 0, (t, r["summary"])
            for k in FRAME_KEYS:
                pfx, nm = k.split("_", 1)
                out[f"{pfx}_t{t}_{nm}"] = r[k]
            out[f"mo_t{t}_off"], out[f"mr_t{t}_obj"] = r["mo_off"], r["mr_obj"]
            if "ev_oldh" in r:
                out[f"ev_t{t}_oldh"], out[f"ev_t{t}_newh"] = r["ev_oldh"], r["ev_newh"]
            tiles.append(m.outputs()["n_tiles"])
        n_int, n_flt, n_rec = int(w["cfg"][1]), int(w["cfg"][2]), int(w["cfg"][5])
        out["final_i"] = np.stack([m.read_prop(p) for p in range(n_int)])
        out["final_f"] = np.stack([m.read_prop(n_int + p) for p in range(n_flt)])
        for r in range(n_rec):
            out[f"final_rec{r}"] = m.read_record(r)
        if m.n_oprops:
            hd = [m.read_object(n_int + n_flt + p) for p in range(m.n_oprops)]
            out["final_oh"], out["final_od"] = np.stack([h for h, _ in hd]), np.stack([d for _, d in hd])
        nx, rm, st = m.read_schedules()
        out["final_s_next"], out["final_s_remain"], out["final_s_present"] = nx, rm, (st & 1).astype(np.uint8)
        stats = m.membership_stats()
        stats["tiles"] = tiles
    finally:
        m.close()
    return out, stats


def report(name, slack, stats, note=""):
    print(f"CHURN_STATS {name} slack={slack} n_full={stats['n_full']} n_seg={stats['n_seg']} "
          f"tiles={min(stats['tiles'])}-{max(stats['tiles'])}{note}")


@pytest.mark.parametrize("slack", [-1, 1, 0, 64])
@pytest.mark.parametrize("name", ["churn", "grow", "tiny_groups", "drain", "burst"])
def test_world_matches_oracle(gpu_available, name, slack):
    """no slack (every change lays the world out again), one slot per 256 (segments overflow and are
    recomputed), the default, and ample slack (changed segments rewritten in place, vacated slots taken
    again): every frame and the final state bit for bit, and the run laid the world out again exactly as
    often as the layout's rule says for this workload (churn_worlds.relayouts)"""
    got, stats = run(cw.world(name), slack)
    report(name, slack, stats)
    compare_runs(got, oracle(name))
    if slack == -1:
        assert stats["n_full"] > 0, stats
    assert (stats["n_full"], stats["n_seg"]) == cw.relayouts(cw.world(name), slack), stats


@pytest.mark.parametrize("slack", [1, 64])
@pytest.mark.parametrize("name", ["churn", "tiny_groups"])
def test_both_relayout_paths_reached(gpu_available, name, slack):
    """membership_stats() after the run: windows applied by rebuilding the segment table (n_full) and
    windows applied by rewriting the changed segments only (n_seg), both.

    Observed on an MI355X (n_full / n_seg): tiny_groups slack 1: 60 / 3, slack 64: 59 / 4; churn slack 1:
    78 / 1, slack 64: 33 / 46.  At slack 1 a segment has max(2, ...) = 2 free slots after a layout
    (nfgpu_host.hip seg_slack), so a segment window needs every segment to gain at most 2: churn has one
    group a scene (8 segments with the groups SwitchScene creates) to have such a window at all."""
    _, stats = run(cw.world(name), slack)
    report(name, slack, stats, " (reach)")
    assert stats["n_full"] > 0 and stats["n_seg"] > 0, stats


@PATHS
def test_every_tick_path(gpu_available, monkeypatch, path):
    """tiny_groups against the oracle and the `churn` golden against the compiled reference's recorded
    frames (tests/golden/gen_churn_golden.py), on the hipRTC kernel, the library kernel and k_tick_touch"""
    set_path(monkeypatch, path)
    compare_runs(run_gpu(cw.world("tiny_groups")), oracle("tiny_groups"))
    w = nfio.read(os.path.join(GOLDEN, "churn.workload.nfio"))
    expected = nfio.read(os.path.join(GOLDEN, "churn.expected.nfio"))
    assert int(w["cfg"][7]) == cw.GOLDEN_TICKS
    compare_runs(run_gpu(w), expected)


@pytest.mark.parametrize("name", ["grow", "churn", "tiny_groups"])
def test_device_guid_lookups(gpu_available, monkeypatch, name):
    """NFGPU_DEV_LOOKUP=1: every batch's lookups on the device mirror of the NFGUID table, which goes
    through rehashes (grow: 300 -> 1245 live) and backward-shift erases between batches"""
    monkeypatch.setenv("NFGPU_DEV_LOOKUP", "1")
    compare_runs(run_gpu(cw.world(name)), oracle(name))


def test_grow_with_parallel_call_folding(gpu_available, monkeypatch):
    monkeypatch.setenv("NFGPU_PAR_CALLS", "8")
    monkeypatch.setenv("NFGPU_HOST_THREADS", "4")
    compare_runs(run_gpu(cw.world("grow")), oracle("grow"))


def test_consumer_reads_every_frame_of_churn(gpu_available):
    """test_gpu_rank_in_tick.run_frames (nfk_outputs_get and the base arrays read after every frame) on
    churn with ample slack and with none: both equal the oracle, their events, fired lists and
    recipients are equal array for array, and the tile count changes over each run"""
    w = cw.world("churn")
    a, tiles_a, _ = run_frames(w, 64)
    b, tiles_b, _ = run_frames(w, -1)
    print(f"CHURN_STATS churn consumer tiles slack64={min(tiles_a)}-{max(tiles_a)} noslack={min(tiles_b)}-{max(tiles_b)}")
    compare_runs(a, oracle("churn"))
    compare_runs(b, oracle("churn"))
    keys = [k for k in a if k.split("_")[0] in ("ev", "re", "fi", "mo", "mr", "final")]
    assert len(keys) == 13 * int(w["cfg"][7]) + 6
    compare_runs({k: a[k] for k in keys}, {k: b[k] for k in keys})
    assert len(set(tiles_a)) > 1 and len(set(tiles_b)) > 1, (tiles_a, tiles_b)


# ---- the state between frames ----
def used_masks(w, t):
    """record 0's used-row masks after window t's calls: the creation-time masks (none for an object
    created later) under the AddRow (first unused row for -1) / Remove / ClearRecord calls"""
    used = [int(x) for x in w["rec0_used"]]
    rows = int(w["rec_rows"][0])
    if "r_op" not in w:
        return used
    for i in np.nonzero(w["r_tick"] <= t)[0]:
        o, op, row = int(w["r_obj"][i]), int(w["r_op"][i]), int(w["r_row"][i])
        if op == 1:
            if row < 0:
                free = [r for r in range(rows) if not (used[o] >> r) & 1]
                if not free:
                    continue
                row = free[0]
            used[o] |= 1 << row
        elif op == 2:
            used[o] &= ~(1 << row)
        elif op == 3:
            used[o] = 0
    return used


class Between:
    """a churn world replayed through test_gpu_scene_query.Driver; at a checkpoint — after frame t, or
    in the middle of window t + 1 — the device's scene queries over the helper's membership and, for a
    sample of live objects, its record finds and enter snapshots over the oracle's state after frame t"""

    def __init__(self, name, slack):
        self.name, self.w = name, cw.world(name)
        self.ms = cw.membership(self.w)
        self.d = Driver(self.w, slack)
        self.m = self.d.m
        self.n_rec = int(self.w["cfg"][5])
        self.n_op = int(self.w["n_oprops"][0]) if "n_oprops" in self.w else 0
        self.rng = np.random.default_rng(3)
        self.n_lists = self.n_snaps = self.n_finds = self.n_reused = self.n_empty = 0

    def scene_state(self, st, t, tag):
        """every pair's player and other lists in the reference's order, whether the pair exists, and
        the online counts; st: the Driver's model State, t: the window whose calls are in"""
        m, ms = self.m, self.ms
        assert np.array_equal(st.alive, ms.alive[t]), tag   # (the Driver and the helper agree)
        cases = []
        for p, (sc, gr) in enumerate(ms.pairs):
            n = int(ms.counts[t, p])
            for who in (True, False):
                found, lst = sqm.get_group_object_list(st, sc, gr, who)
                cases.append((query(sc, gr, Q_PLAYERS if who else Q_OTHERS), lst, found))
            both = sum(len(c[1]) for c in cases[-2:])
            assert both == n, (tag, sc, gr)
            self.n_empty += n == 0 and cases[-1][2]    # a pair that exists with nobody in it
            assert m.GetSceneOnLineCount(sc, gr) == sqm.get_scene_online_count(st, sc, gr), (tag, sc, gr)
        cases.append((query(1, 99, Q_PLAYERS), [], False))
        got, ex = m.query_objects([c[0] for c in cases], with_exists=True)
        for c, g, e in zip(cases, got, ex):
            assert g.tolist() == np.asarray(c[1]).tolist(), f"{tag}: list of {c[0].scene, c[0].group} differs"
            assert bool(e) == c[2], f"{tag}: exists"
            self.n_lists += len(g)
        for sc in sorted({p[0] for p in ms.pairs}):
            assert m.GetSceneOnLineCount(sc) == sqm.get_scene_online_count(st, sc), tag
            assert m.query_objects([query(sc)])[0].tolist() == sqm.get_scene_online_list(st, sc).tolist(), tag
        assert m.GetOnLineCount() == sqm.get_online_count(st), tag

    def model_after(self, t):
        """the enter-snapshot Model over the oracle's state after frame t"""
        w = self.w
        ref = run_oracle(cw.truncated(w, t + 1))
        N = len(w["guid_head"])
        parts = [ref["final_i"].view(np.uint64), ref["final_f"].view(np.uint64)]
        ph = np.zeros((max(self.n_op, 1), N), np.uint64)
        if self.n_op:
            parts.append(ref["final_od"].view(np.uint64))
            ph = ref["final_oh"].view(np.uint64).copy()
        pv = np.concatenate(parts).copy()
        recs = [[] for _ in range(N)]
        if self.n_rec:
            cells, used = ref["final_rec0"], used_masks(w, t)
            types = [int(x) for x in w["rec_ctype"][0][:cells.shape[1]]]
            recs = [[Record(cells.shape[2], types, used[o], cells[o])] for o in range(N)]
        rflags = w["rec_flags"] if self.n_rec else np.zeros((2, 0), np.uint8)
        return Model(N_INT, N_FLT, self.n_op, w["prop_flags"], rflags, w["cls"], pv, ph, recs)

    def object_state(self, mod, objs, tag, on_device):
        """both views' snapshots of objs and one find per object and int column against the model"""
        m, w = self.m, self.w
        objs = np.asarray(objs, np.int64)
        if not len(objs):
            return
        o2, v2 = np.repeat(objs, 2), np.tile([PUB, PRIV], len(objs)).astype(np.uint8)
        stats = {}
        s = m.snapshot_objects(w["guid_head"][o2], w["guid_data"][o2], v2, stats=stats)
        mod.check(s, o2.tolist(), v2.tolist(), tag)
        if on_device:
            assert stats["n_host"] == 0, (tag, stats)
        self.n_snaps += len(o2)
        if self.n_rec:
            for col in (0, 1):
                rows = self.rng.integers(0, int(w["rec_rows"][0]), len(objs))
                bits = np.array([mod.recs[o][0].cells[col, r] for o, r in zip(objs, rows)], np.uint64)
                got = m.find_rows(w["guid_head"][objs], w["guid_data"][objs], np.zeros(len(objs)), np.full(len(objs), col), bits)
                want = [mod.recs[o][0].mask(col, b) for o, b in zip(objs, bits)]
                assert [int(x) for x in got] == want, f"{tag}: find_rows column {col}"
                self.n_finds += len(objs)

    def sample(self, t, pool):
        """up to 96 of pool, the objects in a pair somebody left before first"""
        pool = np.asarray(pool, np.int64)
        re = pool[self.ms.reused[t][pool]]
        rest = pool[~self.ms.reused[t][pool]]
        pick = np.concatenate([re, rest])[:96]
        self.n_reused += int(self.ms.reused[t][pick].sum())
        return pick

    def run(self, every=8):
        w, ms, d = self.w, self.ms, self.d
        nt = int(w["cfg"][7])
        born = d.born
        mod = [None]
        # the checkpoints: every 8th frame, and the frame before a window that joins a drained pair again
        # (the pair exists with nobody in it after the frame and has members in the middle of the window)
        points = set(range(0, nt - 1, every)) | {t - 1 for p in ms.drained() for t in ms.refilled_at(p)}

        def mid(st, t):
            if mod[0] is None:
                return
            self.scene_state(st, t, f"{self.name} window {t}")
            # the objects no call of this window touches hold the state after the last frame; the
            # ones created in it hold their creation-time values and empty records (the arrivals' rows)
            touched = np.zeros(len(born), bool)
            for key, tick in (("x_obj", "x_tick"), ("r_obj", "r_tick"), ("sw_obj", "sw_tick"), ("d_obj", "d_tick")):
                if key in w:
                    touched[w[key][w[tick] == t]] = True
            new = np.nonzero((born == t) & ~touched)[0]
            md = mod[0]
            for o in new:
                md.pv[:N_INT, o] = w["init_i"][:, o].astype(np.int64).view(np.uint64)
                md.pv[N_INT:N_INT + N_FLT, o] = w["init_f"][:, o].view(np.uint64)
                if self.n_op:
                    md.pv[N_INT + N_FLT:, o] = w["init_od"][:, o].view(np.uint64)
                    md.ph[:, o] = w["init_oh"][:, o].view(np.uint64)
                if self.n_rec:
                    md.recs[o][0] = Record(md.recs[o][0].rows, md.recs[o][0].types)
            md.memo = {}
            old = np.nonzero(ms.alive[t - 1] & ms.alive[t] & ~touched)[0]
            self.object_state(md, np.concatenate([new, self.sample(t, old)]), f"{self.name} window {t}", False)
            mod[0] = None
        try:
            for t in range(nt):
                d.frame(t, lambda st, t=t: mid(st, t))
                if t in points:
                    self.scene_state(d.state(t), t, f"{self.name} frame {t}")
                    mod[0] = self.model_after(t)
                    self.object_state(mod[0], self.sample(t, np.nonzero(ms.alive[t])[0]), f"{self.name} frame {t}", True)
            stats = self.m.membership_stats()
            stats["tiles"] = [self.m.outputs()["n_tiles"]]
        finally:
            self.m.close()
        return stats


@pytest.mark.parametrize("name,slack", [("tiny_groups", 1), ("tiny_groups", 64), ("drain", 0), ("drain", 64)])
def test_state_between_frames(gpu_available, name, slack):
    """every 8th frame and in the middle of the window after it: every (scene, group) pair's lists in
    order, pairs that exist with nobody in them, the online counts; the record finds and both enter
    views of live objects, those first that sit where another object was — and of the objects the
    window created, before their first frame"""
    b = Between(name, slack)
    stats = b.run()
    report(name, slack, stats, f" between-frames lists={b.n_lists} snapshots={b.n_snaps} finds={b.n_finds} "
                               f"reused={b.n_reused} empty_pairs={b.n_empty}")
    assert b.n_lists > 1000 and b.n_snaps > 1000 and b.n_reused > 200 and b.n_empty > 0
    assert b.n_finds > 1000 or not b.n_rec


# ---- the arrivals' row buffer ----
def test_two_spawn_batches_past_the_arrival_rows(gpu_available):
    """one window, two nfk_spawn_objects calls of 700 objects: the second outgrows the arrivals' 1024
    rows while the first batch's rows are in them.  Before Execute the first batch reads back
    (GetPropertyInt, get_props, get_record cells, both snapshot views); after the frame and the one
    after it, every output and the whole state equal a twin world's that got the 1400 in one call."""
    w = workload.make_world(n_obj=600, n_scenes=2, groups_per_scene=3, players_per_group=4, n_ticks=3, seed=21,
                            records=True, rec_rows=8, ext_frac=0.05, host_ops=True)
    n0, n_new, half = 600, 1400, 700
    rng = np.random.default_rng(9)
    gh = np.full(n_new, 7, np.int64)
    gd = (np.int64(1) << 41) + np.arange(n_new, dtype=np.int64) * 3 + 1     # (above make_world's 2^40 range)
    scene = rng.integers(1, 3, n_new).astype(np.int32)
    group = rng.integers(1, 5, n_new).astype(np.int32)                        # group 4: a new one
    player = (rng.random(n_new) < 0.2).astype(np.uint8)
    props = np.zeros((n_new, N_INT + N_FLT), np.uint64)
    k = np.arange(n_new)[:, None] * 32 + np.arange(N_INT + N_FLT)[None, :]
    props[:, :N_INT] = (1000 + k[:, :N_INT]).astype(np.uint64)                # all distinct
    props[:, N_INT:] = (k[:, N_INT:] + 0.5).astype(np.float64).view(np.uint64)
    props[:, PID["SceneID"]], props[:, PID["GroupID"]] = scene, group
    props[:, PID["MAXHP"]] += 1 << 20                                        # (HP stays below MAXHP)
    pids = np.arange(N_INT + N_FLT)

    def world(batches):
        m = kernel.world_from_workload(w, capacity=n0 + n_new, slack_per_256=0)
        out = [kernel.run_workload(m, w, 0)]
        for a, b in batches:
            m.spawn_objects(gh[a:b], gd[a:b], scene[a:b], group[a:b], player[a:b], player[a:b], props[a:b])
        return m, out

    def after(m, out):
        sel = np.arange(0, n_new, 3)
        m.add_schedules(gh[sel], gd[sel], np.full(len(sel), workload.KID["HPRegen"]), np.full(len(sel), 0.05, np.float32),
                        np.full(len(sel), -1), np.full(len(sel), int(w["tick_time"][0])))
        for t in (1, 2):
            out.append(kernel.run_workload(m, w, t))
        st = {"i": np.stack([m.read_prop(p) for p in range(N_INT)]), "f": np.stack([m.read_prop(N_INT + p) for p in range(N_FLT)]),
              "rec": m.read_record(0)}
        st["next"], st["remain"], st["present"] = m.read_schedules()
        return st

    m1, out1 = world([(0, half), (half, n_new)])
    m2, out2 = world([(0, n_new)])
    try:
        assert m1.n_obj == n0 + n_new
        # the first batch, read back in the window it arrived in
        first = np.arange(half)
        for o in (0, 1, half - 1):
            assert m1.GetPropertyInt((7, int(gd[o])), "Gold") == int(props[o, PID["Gold"]])
            assert m1.GetPropertyFloat((7, int(gd[o])), "X") == float(props[o, PID["X"]:PID["X"] + 1].view(np.float64)[0])
        got = m1.get_props(np.repeat(gh[first], len(pids)), np.repeat(gd[first], len(pids)), np.tile(pids, half))
        assert np.array_equal(got.reshape(half, -1), props[:half])
        cells = m1.get_records(gh[first], gd[first], np.zeros(half), rng.integers(0, 8, half), rng.integers(0, 3, half))
        assert not cells.any()                                               # empty records: unused rows read 0
        recs = [[Record(8, [int(x) for x in w["rec_ctype"][0][:3]])] for _ in range(n_new)]
        mod = Model(N_INT, N_FLT, 0, w["prop_flags"], w["rec_flags"], player, props.T.copy(), np.zeros((1, n_new), np.uint64), recs)
        some = np.concatenate([first[:40], first[-40:], [half, n_new - 1]])
        o2, v2 = np.repeat(some, 2), np.tile([PUB, PRIV], len(some)).astype(np.uint8)
        mod.check(m1.snapshot_objects(gh[o2], gd[o2], v2), o2.tolist(), v2.tolist(), "arrivals, before their frame")
        st1, st2 = after(m1, out1), after(m2, out2)
        for t, (a, b) in enumerate(zip(out1, out2)):
            assert a["summary"]["device_error"] == 0
            for key in FRAME_KEYS + ("mo_off", "mr_obj"):
                assert np.array_equal(a[key], b[key]), (t, key)
        assert len(out1[1]["ev_obj"]) > 0 and np.any(out1[2]["fi_obj"] >= n0)
        for key in st1:
            assert np.array_equal(st1[key].view(np.uint8), st2[key].view(np.uint8)), key
        # what no program and no call writes is the creation value still (Level, DEF_VALUE, AtkDis)
        for p in (PID["Level"], PID["DEF_VALUE"]):
            assert np.array_equal(st1["i"][p][n0:].view(np.uint64), props[:, p])
        assert np.array_equal(st1["f"][PID["AtkDis"] - N_INT][n0:].view(np.uint64), props[:, PID["AtkDis"]])
        # and the old world is the oracle's (the arrivals are beside it, in cells of their own or not)
        for p in (PID["Level"], PID["DEF_VALUE"]):
            assert np.array_equal(st1["i"][p][:n0], run_oracle(w)["final_i"][p])
    finally:
        m1.close()
        m2.close()


@pytest.mark.parametrize("slack", [-1, 64])
def test_cpp_plugin_replay_tiny_groups(gpu_available, tmp_path, slack):
    """tiny_groups through the C++ plugin (tests/cpp/plugin_replay.cpp, as
    test_gpu_parity.py::test_cpp_plugin_replay_create_destroy): CreateObject, DestroyObject, SwitchScene
    and the record row calls of 64 windows through its buffers, its world laid out with no slack and
    with ample slack (SetSlackPer256)"""
    exe = os.path.join(ROOT, "tests", "cpp", "_bin", "plugin_replay")
    w = cw.world("tiny_groups")
    wp, op = str(tmp_path / "w.nfio"), str(tmp_path / "o.nfio")
    nfio.write(wp, w)
    subprocess.run([exe, wp, op, str(slack)], check=True, timeout=300)
    got, ref = nfio.read(op), dict(oracle("tiny_groups"))
    for t in range(int(w["cfg"][7])):   # functors in NFGUID order: compared in (object, kind) order
        o = np.lexsort((got[f"fi_t{t}_kind"], got[f"fi_t{t}_obj"]))
        r = np.lexsort((ref[f"fi_t{t}_kind"], ref[f"fi_t{t}_obj"]))
        for k in ("obj", "kind", "rem"):
            got[f"fi_t{t}_{k}"], ref[f"fi_t{t}_{k}"] = got[f"fi_t{t}_{k}"][o], ref[f"fi_t{t}_{k}"][r]
    assert sum(int(np.sum(ref[f"re_t{t}_rrc"] >> 24 != 0)) for t in range(int(w["cfg"][7]))) > 100   # row events
    compare_runs({k: v for k, v in got.items() if not k.startswith("rank_")}, {k: v for k, v in ref.items() if k in got})
