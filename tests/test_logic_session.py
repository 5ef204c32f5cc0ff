"""Game logic written against the reference's interfaces (tests/cpp/logic_session.cpp) on two servers:
the reference's own NFCKernelModule + NFCScheduleModule (logic_session_ref, CPU) and the reference-side
GPU plugin (integration/NFGPUKernelPlugin.cpp over libnfgpu, logic_session).  The logic registers
per-object callbacks (NFIKernelModule::AddPropertyCallBack / AddRecordCallBack, NFIKernelModule.h:28-45),
writes device state both through NFIKernelModule and straight through the objects
(GetObject(self)->SetProperty*, FindRecord(self, r)->SetInt / AddRow / Remove), and runs Tutorial3's own
sequence (HelloWorld3Module.cpp: class callback, functor-only OnHeartBeat, dynamic Hello / World
properties with per-object callbacks, DoEvent).  Compared frame by frame:

* the heartbeat functors, Tutorial3's callback lines, and every object's properties and rec0 cells read
  through the HOST objects and through NFIKernelModule: equal;
* per-object callbacks of the window's calls (phase 0): the same sequence;
* per-object callbacks fired by Execute (phase 1): the same sequence — one callback per accepted Set
  of the heartbeat programs (the reference's functors' Sets; on the GPU plugin the device's per-Set
  log, k_chain), objects in NFGUID order, each object's schedules in name order, each program's ops
  and a record op's rows in order (SM:52-80);
* with Poison able to kill (workload lethal_poison: HP -> 0 -> 3 within one program), the kills of an
  NFCNPCRefreshModule::OnObjectHPEvent-style callback (newVar <= 0, NFCNPCRefreshModule.cpp:113-124)
  and the OnDeadDestroyHeart heartbeats it adds: the same;
* (logic_mode, tests/cpp/logic_session.cpp) functors reading other objects' program-written properties
  (the reference's walk order, SM:52-80: with NFGPUKernelModule::SetWalkOrderReads equal, without it the
  documented divergence — the frame's values — asserted exactly); components that destroy their own
  object (deferred to the next Execute, KM:275-279) or another one (at once); NFCNPCRefreshModule's own
  callback pattern (an HP callback on every NPC, NFCNPCRefreshModule.cpp:104) at 20k objects."""
import os
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import nfio, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "oracle", "_ref", "logic_session")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "logic_session_ref")


def _world(seed, n_obj=1200, n_ticks=12, lethal=False, set_ops=False, logic_mode=0, groups_per_scene=3,
           const_guards=False):
    w = workload.make_world(n_obj=n_obj, n_scenes=2, groups_per_scene=groups_per_scene, players_per_group=4, n_ticks=n_ticks,
                            tick_ms=1000, seed=seed, ext_frac=0.05, host_ops=True, rmw_frac=0.02, spawn_frac=0.02,
                            destroy_frac=0.02, records=True, rec_rows=16, rec_float_op=False, rec_set_frac=0.03,
                            rec_set_float=False, rec_row_frac=0.02, lethal_poison=lethal, set_ops=set_ops,
                            const_guards=const_guards)
    # an int-only record (the reference's NFCRecord::SetFloat cannot hold an f64 cell, test_oracle.py):
    # the charge column becomes an int column with the same bits; no program touches it
    w["rec_ctype"] = np.zeros_like(w["rec_ctype"])
    if logic_mode:
        w["logic_mode"] = np.array([logic_mode], np.int64)
    return w


def _run(exe, w, tmp_path, tag, env=None):
    wp, op = str(tmp_path / f"{tag}_w.nfio"), str(tmp_path / f"{tag}_o.nfio")
    nfio.write(wp, w)
    subprocess.run([exe, wp, op], check=True, timeout=600, env=None if env is None else {**os.environ, **env})
    return nfio.read(op)


def _chains(out, t, pfx, key):
    """Per-object callbacks of frame t as {phase: [(obj, key, old, new), ...]} in firing order."""
    ph = np.asarray(out[f"{pfx}_t{t}_phase"])
    rows = list(zip(out[f"{pfx}_t{t}_obj"], out[f"{pfx}_t{t}_{key}"], out[f"{pfx}_t{t}_old"], out[f"{pfx}_t{t}_new"]))
    return {p: [tuple(int(x) for x in r) for r, q in zip(rows, ph) if q == p] for p in (0, 1)}


def _coalesce(seq):
    """(obj, key) -> (first old, last new) over the phase's callbacks (what one callback per
    (object, property) and frame would report)"""
    first, last = {}, {}
    for o, k, a, b in seq:
        first.setdefault((o, k), a)
        last[(o, k)] = b
    return {key: (first[key], last[key]) for key in first}


def _cell_history(got, ref, t, flat, w):
    """(diagnosis) the record callbacks of the object owning rec0 cell `flat` up to frame t, both sides"""
    rows, cols = int(w["rec_rows"][0]), int(w["rec_cols"][0])
    o, rem = divmod(int(flat), cols * rows)
    c, row = divmod(rem, rows)
    h = {}
    for name, out in (("gpu", got), ("ref", ref)):
        h[name] = [(u, int(ph), int(rrc) >> 24, (int(rrc) >> 8) & 255, int(rrc) & 255, int(a), int(b))
                   for u in range(t + 1)
                   for ph, ob, rrc, a, b in zip(out[f"rc_t{u}_phase"], out[f"rc_t{u}_obj"], out[f"rc_t{u}_rrc"],
                                                out[f"rc_t{u}_old"], out[f"rc_t{u}_new"])
                   if ob == o and (((int(rrc) >> 8) & 255) == row or int(rrc) >> 24)]
    return {"obj": o, "row": row, "col": c, **h}


def _t3(out, t):
    return bytes(np.asarray(out[f"t3_t{t}_log"], np.uint8)).decode()


def test_logic_session_reference_runs_tutorial3(tmp_path):
    """CPU: the logic on the reference's own modules — Tutorial3's sequence (its class callback, the
    per-object callbacks on the dynamic World / Hello properties, DoEvent's handler whose
    SetPropertyInt on the string property is refused) and its functor-only OnHeartBeat firing every
    5 s with the remaining count."""
    if not os.path.exists(REF_EXE):
        pytest.skip("logic_session_ref not built (needs /root/reference at build time)")
    w = _world(71, n_obj=300)
    out = _run(REF_EXE, w, tmp_path, "ref")
    setup = bytes(np.asarray(out["t3_setup"], np.uint8)).decode().splitlines()
    assert any("OnClassCallBackEvent Player 10" in s for s in setup)
    assert "-1 OnPropertyCallBackEvent 10 World 0 1111" in setup
    assert "-1 OnPropertyStrCallBackEvent 10 Hello  hello,World" in setup
    assert "-1 OnEvent sets 01" in setup and "-1 OnPropertyStrCallBackEvent 10 Hello hello,World 200" in setup
    hb = [ln for t in range(int(w["cfg"][7])) for ln in _t3(out, t).splitlines() if "OnHeartBeat 0-10 " in ln]
    # next = start + 5000 * (all - remain) after each fire (SM:71-72): the first fire leaves next
    # where it was, so the schedule fires on frames 5, 6 (start + 5 s) and 10 (start + 10 s)
    assert hb == [f"{t} OnHeartBeat 0-10 OnHeartBeat 5.000000 {c}" for t, c in ((5, 9), (6, 8), (10, 7))]
    assert any("OnEvent 1 10 1003 s3" in ln for ln in _t3(out, 3).splitlines())


def test_logic_session_reference_kills_within_a_frame(tmp_path):
    """CPU: with lethal Poison the reference's per-object HP callbacks see HP reach 0 and come back
    within one frame (its functor's two Sets), so OnObjectHPEvent kills objects whose frame ends alive —
    what a callback fired once per (object, property) and frame would miss."""
    if not os.path.exists(REF_EXE):
        pytest.skip("logic_session_ref not built (needs /root/reference at build time)")
    w = _world(73, n_obj=600, lethal=True)
    out = _run(REF_EXE, w, tmp_path, "ref")
    hp = workload.PID["HP"]
    hidden = kills = 0
    for t in range(int(w["cfg"][7])):
        kills += len(bytes(np.asarray(out[f"k_t{t}_kills"], np.uint8)).decode().splitlines())
        chain = _chains(out, t, "pc", "pid")[1]
        co = _coalesce([r for r in chain if r[1] == hp])
        dead = {o for o, k, a, b in chain if k == hp and np.int64(np.uint64(b)) <= 0}
        hidden += sum(1 for o in dead if np.int64(np.uint64(co[(o, hp)][1])) > 0)
    assert kills > 20 and hidden > 20, (kills, hidden)


def _lines(out, key):
    return bytes(np.asarray(out[key], np.uint8)).decode().splitlines()


def test_logic_session_reference_components_destroy(tmp_path):
    """CPU: components (NFIComponent, run in NFCKernelModule::Execute's object walk, KM:88-95) on the
    reference's own modules: DestroyObject of the component's own object is deferred to the next Execute
    (KM:275-279: DestroySelf puts it on mtDeleteSelfList, applied at KM:76-84), of another object applied at
    once — the sequence the adapter must reproduce (its walk over a copy of the objects with components,
    ADVICE r5)."""
    if not os.path.exists(REF_EXE):
        pytest.skip("logic_session_ref not built (needs /root/reference at build time)")
    w = _world(75, n_obj=1200, logic_mode=4)
    out = _run(REF_EXE, w, tmp_path, "ref")
    nt = int(w["cfg"][7])
    gone_at = {}
    for t in range(nt):
        for ln in _lines(out, f"k_t{t}_comp"):
            if ln.startswith("gone "):
                gone_at[int(ln.split()[1])] = t
    n_self = n_other = 0
    for t in range(nt):
        for ln in _lines(out, f"k_t{t}_comp"):
            if not ln.startswith("destroy "):
                continue
            me, victim, ok = (int(x) for x in ln.split()[1:])
            assert ok == 1
            if me == victim:  # deferred: gone after the NEXT Execute
                n_self += 1
                assert gone_at.get(victim) == (t + 1 if t + 1 < nt else None), ln
            else:
                n_other += 1
                assert gone_at.get(victim) == t, ln
    assert n_self >= 5 and n_other >= 5, (n_self, n_other)


@pytest.mark.gpu
# seed 74: the set_ops programs (assignments, guards against 0 and against another int property)
# seed 75: logic_mode 1 | 2 | 4 — cross-object functor reads answered in walk order, components destroying
# objects (their own deferred), with lethal Poison
# seed 79: guards against constants other than 0 (NFK_GUARD_K; mode 32 = the const_guards programs)
# seed 78: logic_mode 16 — only EXP watched with the set_ops programs: the per-Set log re-runs the earlier kinds
# whose writes a watched Set reads (Patrol's SP / Camp, HPRegen's HP before Poison's EXP ops)
@pytest.mark.parametrize("seed,lethal,set_ops,mode", [(71, False, False, 0), (72, False, False, 0), (73, True, False, 0),
                                                      (74, False, True, 0), (75, True, False, 7), (78, False, True, 16),
                                                      (79, False, False, 32)])
def test_logic_session_gpu_plugin_matches_reference(gpu_available, tmp_path, seed, lethal, set_ops, mode):
    if not (os.path.exists(GPU_EXE) and os.path.exists(REF_EXE)):
        pytest.skip("logic_session not built (needs /root/reference at build time)")
    w = _world(seed, lethal=lethal, set_ops=set_ops, logic_mode=mode & ~32, const_guards=bool(mode & 32))
    got, ref = _run(GPU_EXE, w, tmp_path, "gpu"), _run(REF_EXE, w, tmp_path, "ref")
    nt = int(w["cfg"][7])
    if mode & 7:
        n_xr = 0
        for t in range(nt):
            assert _lines(got, f"k_t{t}_comp") == _lines(ref, f"k_t{t}_comp"), t
            for k in ("obj", "kind", "peer", "hp", "x", "mp", "self"):
                np.testing.assert_array_equal(got[f"xr_t{t}_{k}"], ref[f"xr_t{t}_{k}"], err_msg=f"xr_t{t}_{k}")
            n_xr += len(ref[f"xr_t{t}_obj"])
        assert n_xr > 1000 and sum(len(_lines(ref, f"k_t{t}_comp")) for t in range(nt)) > 10
    assert bytes(np.asarray(got["t3_setup"], np.uint8)) == bytes(np.asarray(ref["t3_setup"], np.uint8))
    n_obj_cb = n_rec_cb = 0
    n_kills = 0
    for t in range(nt):
        assert _t3(got, t) == _t3(ref, t), t
        for k in ("k_t{}_kills", "k_t{}_dead"):  # OnObjectHPEvent's kills, OnDeadDestroyHeart's calls
            assert bytes(np.asarray(got[k.format(t)], np.uint8)) == bytes(np.asarray(ref[k.format(t)], np.uint8)), k.format(t)
        n_kills += len(bytes(np.asarray(ref[f"k_t{t}_kills"], np.uint8)).decode().splitlines())
        fo = lambda o: sorted(zip(o[f"fi_t{t}_obj"], o[f"fi_t{t}_kind"], o[f"fi_t{t}_rem"]))
        assert fo(got) == fo(ref), t
        for k in ("v_t{}_host", "v_t{}_kernel", "r_t{}_kcells", "r_t{}_cells", "r_t{}_used"):
            g_, r_ = np.asarray(got[k.format(t)]), np.asarray(ref[k.format(t)])
            bad = np.nonzero(g_ != r_)[0]
            assert len(bad) == 0, (k.format(t), [(int(i), int(g_[i]), int(r_[i])) for i in bad[:8]],
                                   _cell_history(got, ref, t, bad[0], w) if k.startswith("r") else None)
        # the host objects agree with NFIKernelModule's reads (the device's, on the GPU plugin)
        np.testing.assert_array_equal(got[f"v_t{t}_host"], got[f"v_t{t}_kernel"])
        for pfx, key in (("pc", "pid"), ("rc", "rrc")):
            g, r = _chains(got, t, pfx, key), _chains(ref, t, pfx, key)
            assert g[0] == r[0], (t, pfx)   # the window's calls fire in call order, as in the reference
            assert g[1] == r[1], (t, pfx)   # Execute: one per accepted Set, in the heartbeat walk's order
            if pfx == "pc":
                n_obj_cb += len(g[0]) + len(g[1])
            else:
                n_rec_cb += len(g[0]) + len(g[1])
    assert n_obj_cb > (300 if mode & 16 else 1000) and (n_rec_cb > 100 or mode & 16), (n_obj_cb, n_rec_cb)
    assert n_kills > 20 or not lethal, n_kills
    if mode & 16:  # the seed exercises the dependency: the log of the watched kinds alone differs
        bad = _run(GPU_EXE, w, tmp_path, "gpu_noclosure", env={"NFGPU_CHAIN_NO_CLOSURE": "1"})
        assert any(_chains(bad, t, "pc", "pid")[1] != _chains(ref, t, "pc", "pid")[1] for t in range(nt))


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"NFGPU_JIT": "0"}, {"NFGPU_CHAIN_U": "0"}], ids=["library_chain_u", "touch_chain"])
def test_logic_session_per_set_log_kernels(gpu_available, tmp_path, env):
    """The per-Set log on its other kernels: k_chain_u over the library's DynSchema tables (NFGPU_JIT=0)
    and the written-property-list k_chain (NFGPU_CHAIN_U=0) — the lethal-Poison seed's per-object callbacks
    (HP 5 -> 0 -> 3 inside one program, the kills) and the EXP-only seed's dependency closure, equal to the
    compiled reference as on the default hipRTC k_chain_u."""
    if not (os.path.exists(GPU_EXE) and os.path.exists(REF_EXE)):
        pytest.skip("logic_session not built (needs /root/reference at build time)")
    for seed, lethal, set_ops, mode in ((73, True, False, 0), (78, False, True, 16), (79, False, False, 32)):
        w = _world(seed, lethal=lethal, set_ops=set_ops, logic_mode=mode & ~32, const_guards=bool(mode & 32))
        got, ref = _run(GPU_EXE, w, tmp_path, f"gpu{seed}", env=env), _run(REF_EXE, w, tmp_path, f"ref{seed}")
        n = 0
        for t in range(int(w["cfg"][7])):
            g, r = _chains(got, t, "pc", "pid"), _chains(ref, t, "pc", "pid")
            assert g[1] == r[1], (seed, t)
            assert bytes(np.asarray(got[f"k_t{t}_kills"], np.uint8)) == bytes(np.asarray(ref[f"k_t{t}_kills"], np.uint8))
            n += len(g[1])
        assert n > 300, (seed, n)


@pytest.mark.gpu
def test_logic_session_cross_object_reads_divergence(gpu_available, tmp_path):
    """Without walk-order reads (the plugin's default) a heartbeat functor's read of another object's
    program-written property sees the frame's value — every object's device programs ran before the host
    functors — where the reference's sees it as of its place in the walk (objects in NFGUID order,
    SM:52-80).  Asserted exactly: every read equals that object's value after the frame (read back through
    NFIKernelModule at the frame's end), and the reads differ from the reference's exactly where the peer
    (or, for its own HP, a later schedule name of the reader) made a Set after the reader's place."""
    if not (os.path.exists(GPU_EXE) and os.path.exists(REF_EXE)):
        pytest.skip("logic_session not built (needs /root/reference at build time)")
    w = _world(76, lethal=True, logic_mode=1)
    got, ref = _run(GPU_EXE, w, tmp_path, "gpu"), _run(REF_EXE, w, tmp_path, "ref")
    nt, n = int(w["cfg"][7]), len(w["guid_head"])
    hp, x, mp = workload.PID["HP"], workload.PID["X"], workload.PID["MP"]
    n_diff = n_later = 0
    for t in range(nt):
        vk = np.asarray(got[f"v_t{t}_kernel"]).reshape(-1, n)
        peer = np.asarray(got[f"xr_t{t}_peer"])
        obj = np.asarray(got[f"xr_t{t}_obj"])
        np.testing.assert_array_equal(got[f"xr_t{t}_peer"], ref[f"xr_t{t}_peer"])
        live = peer < n  # (the Tutorial3 object is never a peer)
        alive = vk[workload.PID["MAXHP"], peer[live]] != 0
        for k, p in (("hp", hp), ("x", x), ("mp", mp)):
            g = np.asarray(got[f"xr_t{t}_{k}"])[live]
            np.testing.assert_array_equal(g[alive], vk[p, peer[live][alive]], err_msg=f"xr_t{t}_{k}")
        np.testing.assert_array_equal(np.asarray(got[f"xr_t{t}_self"]), vk[hp, obj], err_msg=f"xr_t{t}_self")
        d = np.asarray(got[f"xr_t{t}_hp"]) != np.asarray(ref[f"xr_t{t}_hp"])
        n_diff += int(d.sum())
        # a peer BEFORE the reader in NFGUID order has made all its Sets in the reference too: equal
        gk = lambda o: (np.asarray(w["guid_head"])[o], np.asarray(w["guid_data"])[o])
        before = np.array([gk(p) < gk(o) for p, o in zip(peer, obj)], bool)
        assert not (d & before).any(), t
        n_later += int((~before).sum())
    assert n_diff > 20 and n_later > 100, (n_diff, n_later)


GOLDEN_NPC = os.path.join(ROOT, "tests", "golden", "logic_npc20k.json")


def _npc20k_world():
    """NFCNPCRefreshModule's callback pattern at 20k objects: an HP callback (and its kill logic) on every
    NPC, nothing else watched, lethal Poison (tests/golden/gen_logic_golden.py)"""
    return _world(77, n_obj=20000, lethal=True, logic_mode=8, groups_per_scene=64)


def logic_digests(out, nt):
    """per frame: sha256 of every logged array (the fired list as sorted triples), for a fixture of the
    reference's run that is too slow to repeat on every GPU run (~4 min of the reference's modules)"""
    import hashlib
    d = {}
    for t in range(nt):
        for k in sorted(out):
            if not k.startswith(("pc_t%d_" % t, "rc_t%d_" % t, "k_t%d_" % t, "v_t%d_" % t, "r_t%d_" % t, "t3_t%d_" % t)):
                continue
            d[k] = hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest()
        fi = np.array(sorted(zip(*(np.asarray(out[f"fi_t{t}_{c}"], np.int64) for c in ("obj", "kind", "rem")))),
                      np.int64)
        d[f"fi_t{t}"] = hashlib.sha256(fi.tobytes()).hexdigest()
        d[f"n_pc_t{t}"] = int(len(out[f"pc_t{t}_obj"]))
    return d


def workload_digest(w):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_logic_session_npc_hp_callbacks_20k(gpu_available, tmp_path):
    """The reference's own per-NPC callback pattern (NFCNPCRefreshModule.cpp:98-105: AddPropertyCallBack(self,
    HP) on every NPC at creation, its OnObjectHPEvent kill logic) at 20k objects through the GPU plugin, equal
    frame by frame to the reference's modules (per-Set HP callbacks in the walk's order, kills, the fired
    lists, every object's properties and record cells through the host objects and NFIKernelModule):
    compared with digests of the reference's run (tests/golden/logic_npc20k.json, made by
    tests/golden/gen_logic_golden.py from logic_session_ref)."""
    if not os.path.exists(GPU_EXE):
        pytest.skip("logic_session not built (needs /root/reference at build time)")
    import json
    gold = json.load(open(GOLDEN_NPC))
    w = _npc20k_world()
    assert workload_digest(w) == gold["workload"], "the generated workload differs from the fixture's"
    got = _run(GPU_EXE, w, tmp_path, "gpu")
    nt = int(w["cfg"][7])
    dg = logic_digests(got, nt)
    bad = [k for k in gold["digests"] if dg.get(k) != gold["digests"][k]]
    assert not bad, bad[:10]
    assert sum(gold["digests"][f"n_pc_t{t}"] for t in range(nt)) > 100000
