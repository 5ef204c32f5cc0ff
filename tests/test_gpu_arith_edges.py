"""GPU: the f64 / int64 effect arithmetic and both Set predicates at their edges (tests/arith_edges.py:
non-dyadic constants, constants a compiler folds, NaN / inf / +-0 / denormals, values on both sides of the
1e-15 and 0.001 thresholds, int64 values that wrap or defeat a 32-bit compare) on every kernel path, bit for
bit against the compiled reference's golden outputs and the oracle; the per-Set log against the predicates;
the host's read-your-writes overlay against a model of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from noahgameframe_amd import kernel, nfio, workload as wl
from tests import arith_edges
from tests.parity import ROOT, compare_runs, run_oracle
from tests.test_gpu_parity import PATHS, set_path

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 3
NO_FUSE = 4096   # kAblNoFuse: the fan-out in k_fanout, after k_tick (outputs exact)

_oracle = {}


def world_and_oracle(name):
    """a builder's world and the oracle's run of it, computed once and shared (never changed)"""
    if name not in _oracle:
        w = arith_edges.BUILDERS[name](SEED)
        _oracle[name] = (w, run_oracle(w))
    return _oracle[name]


def run_gpu(w, path=None):
    """tests.parity.run_gpu, which also checks that the world runs the kernel the path names (a working set
    that did not fit the register slots would run k_tick_touch on every path) and raised no device error"""
    m = kernel.world_from_workload(w)
    if path is not None:
        on, msg = m.jit_status()
        assert path == "k_tick_touch" or on == (path == "k_tick"), (path, msg)
        assert "does not fit" not in msg, msg
    out = {}
    for t in range(int(w["cfg"][7])):
        r = kernel.run_workload(m, w, t)
        assert r["summary"]["device_error"] == 0, r["summary"]
        for k in ("ev_obj", "ev_pid", "ev_old", "ev_new", "re_obj", "re_rrc", "re_old", "re_new",
                  "fi_obj", "fi_kind", "fi_rem"):
            pfx, nm = k.split("_", 1)
            out[f"{pfx}_t{t}_{nm}"] = r[k]
        out[f"mo_t{t}_off"] = r["mo_off"]
        out[f"mr_t{t}_obj"] = r["mr_obj"]
    n_int, n_flt, n_rec = int(w["cfg"][1]), int(w["cfg"][2]), int(w["cfg"][5])
    out["final_i"] = np.stack([m.read_prop(p) for p in range(n_int)])
    out["final_f"] = np.stack([m.read_prop(n_int + p) for p in range(n_flt)])
    for r in range(n_rec):
        out[f"final_rec{r}"] = m.read_record(r)
    nx, rm, st = m.read_schedules()
    out["final_s_next"] = nx
    out["final_s_remain"] = rm
    out["final_s_present"] = (st & 1).astype(np.uint8)
    m.close()
    return out


@PATHS
def test_gpu_arith_matches_reference_golden(gpu_available, monkeypatch, path):
    """tests/golden/arith.*: what the reference's own NFCProperty made of the combined world"""
    set_path(monkeypatch, path)
    w = nfio.read(os.path.join(GOLDEN, "arith.workload.nfio"))
    compare_runs(run_gpu(w, path), nfio.read(os.path.join(GOLDEN, "arith.expected.nfio")))


@PATHS
@pytest.mark.parametrize("name", sorted(arith_edges.BUILDERS))
def test_gpu_arith_matches_oracle(gpu_available, monkeypatch, name, path):
    set_path(monkeypatch, path)
    w, ref = world_and_oracle(name)
    compare_runs(run_gpu(w, path), ref)


@pytest.mark.parametrize("name", ["record_edges", "float_props"])
def test_gpu_arith_matches_oracle_through_k_fanout(gpu_available, monkeypatch, name):
    """the fan-out in k_fanout (kAblNoFuse): the record predicate lives in k_records and in k_rset_slots"""
    monkeypatch.setenv("NFGPU_JIT", "1")
    monkeypatch.setenv("NFGPU_ABLATE", str(NO_FUSE))
    w, ref = world_and_oracle(name)
    compare_runs(run_gpu(w), ref)


# ---- the per-Set log -----------------------------------------------------------------------------
_chains = {}


def chain_log(tmp_path_factory, chain_u):
    """tests/arith_edges_chain.py run once per NFGPU_CHAIN_U setting, each in a process of its own"""
    if chain_u not in _chains:
        out = str(tmp_path_factory.mktemp("chain") / f"chain{chain_u}.npz")
        env = dict(os.environ, NFGPU_CHAIN_U=chain_u, NFGPU_JIT="1", NFGPU_ABLATE="0")
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "arith_edges_chain.py"), out, str(SEED)],
                       check=True, env=env, cwd=ROOT, timeout=300)
        z = np.load(out)
        _chains[chain_u] = {k: z[k] for k in z.files}
    return _chains[chain_u]


def test_per_set_logs_of_both_kernels_are_equal(gpu_available, tmp_path_factory):
    a, b = chain_log(tmp_path_factory, "1"), chain_log(tmp_path_factory, "0")
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("chain_u", ["1", "0"])
@pytest.mark.parametrize("name", ["float_props", "int_edges"])
def test_per_set_log_follows_the_predicates(gpu_available, tmp_path_factory, name, chain_u):
    """every logged Set is one NFCProperty::SetInt / SetFloat accepts (PR:273, PR:314); the Sets of one
    (object, property) link, new to old, bit for bit (a NaN, an infinity, a -0.0 among them); where the
    window's SetProperty calls left the pair alone, the chain starts at the frame event's old value and ends
    at its new one, and a chain that returns to where the frame started has no event"""
    z = chain_log(tmp_path_factory, chain_u)
    w, ref = world_and_oracle(name)
    n_int = int(w["cfg"][1])
    n_log = n_link = n_ev = n_back = n_odd = 0
    for t in range(int(w["cfg"][7])):
        obj, pid, old, new = (z[f"{name}_t{t}_{k}"] for k in ("obj", "pid", "old", "new"))
        assert set(pid.tolist()) <= set(arith_edges_watch())
        isf = pid >= n_int
        with np.errstate(invalid="ignore", over="ignore"):
            refused_f = np.abs(new.view(np.float64) - old.view(np.float64)) <= 1e-15
        assert not (isf & refused_f).any(), f"frame {t}: a float Set the predicate refuses is logged"
        assert not (~isf & (new == old)).any(), f"frame {t}: an int Set of the value held is logged"
        f = new[isf].view(np.float64)
        n_odd += int((~np.isfinite(f)).sum() + ((f == 0) & np.signbit(f)).sum())
        chains = {}   # (object, property) -> [first old, last new] of its Sets, in the walk's order
        for i, key in enumerate(zip(obj.tolist(), pid.tolist())):
            if key in chains:
                assert chains[key][1] == int(old[i]), f"frame {t}: {key}'s Sets do not link"
                chains[key][1] = int(new[i])
                n_link += 1
            else:
                chains[key] = [int(old[i]), int(new[i])]
        sel = np.asarray(w["x_tick"]) == t
        touched = set(zip(np.asarray(w["x_obj"])[sel].tolist(), np.asarray(w["x_pid"])[sel].tolist()))
        ev = {(int(o), int(p)): (int(a), int(b)) for o, p, a, b in
              zip(*(z[f"{name}_t{t}_ev_{k}"] for k in ("obj", "pid", "old", "new")))}
        for key, c in chains.items():
            if key in touched:
                continue
            if c[0] == c[1]:
                assert key not in ev, f"frame {t}: {key} returned to its frame-start bits and has an event"
                n_back += 1
            else:
                assert ev.get(key) == (c[0], c[1]), f"frame {t}: {key}'s chain and event differ"
                n_ev += 1
        watched_ev = {k for k in ev if k[1] in arith_edges_watch() and k not in touched}
        assert watched_ev <= set(chains), f"frame {t}: an event of a watched property without a logged Set"
        n_log += len(obj)
        # the frame's events are the oracle's (the log rides on a frame that is right)
        assert np.array_equal(z[f"{name}_t{t}_ev_new"], ref[f"ev_t{t}_new"])
    print(name, "logged", n_log, "links", n_link, "with event", n_ev, "returned", n_back, "nan/inf/-0", n_odd)
    assert n_log > 1000 and n_link > 100 and n_ev > 500
    if name == "float_props":
        assert n_odd > 20, "no NaN, infinity or -0.0 went through the log"


def arith_edges_watch():
    return [wl.PID[p] for p in wl.FLT_PROPS + ["HP", "SP"]]


# ---- the host's read-your-writes overlay ----------------------------------------------------------
def accepts_float(cur, v):
    """NFCProperty::SetFloat (PR:314): refused when IsZeroDouble(v - cur), |d| <= 1e-15 (never with a NaN)"""
    return not abs(v - cur) <= 1e-15


def accepts_record_float(cur, v):
    """NFCRecord::SetFloat with TData::operator== (NFIDataList.h:106-113): |d| < 0.001 is equal"""
    d = v - cur
    return not (d < 0.001 and d > -0.001)


def bits(x):
    return wl.f64bits(x) & 0xFFFFFFFFFFFFFFFF


def replay(start, calls, accepts):
    """calls on one value: the value each Get after a call reads, and the event the frame's dirty diff
    makes of them — (first old, last new) of the accepted Sets, dropped when the bits are unchanged (a NaN
    set over the same NaN, a value set away and back)"""
    cur, first, reads = start, None, []
    for v in calls:
        if accepts(cur, v):
            first = cur if first is None else first
            cur = v
        reads.append(cur)
    ev = None if first is None or bits(first) == bits(cur) else (bits(first), bits(cur))
    return reads, ev


def test_read_your_writes_overlay_at_the_predicates_edges(gpu_available):
    """nfgpu_host.hip keeps host copies of both predicates for GetProperty / GetRecord between a Set and the
    frame that applies it.  Calls on one f64 property and one f64 cell, a Get after each: every Get equals
    the model, and after the frame the device's value and the coalesced event do — the host copies, k_sets and
    k_rsets agree at 5e-16 / 2e-15, at 0.000999 / 0.001, on NaN over NaN, -0.0 over NaN, 0.0 over -0.0, inf over
    inf and a denormal."""
    NAN, INF = float("nan"), float("inf")
    w = wl.make_world(n_obj=64, n_scenes=1, groups_per_scene=2, players_per_group=4, n_ticks=2, seed=21, records=True,
                      rec_rows=8, ext_frac=0.0, host_ops=False)
    X, xi = wl.PID["X"], wl.PID["X"] - wl.N_INT
    objs = {"all": 5, "back": 17, "below": 40}
    w["init_f"][xi, list(objs.values())] = 1.25
    ROW, COL = 3, 2
    w["rec0_used"][list(objs.values())] |= np.uint64(1 << ROW)
    w["rec0_cells"][list(objs.values()), COL, ROW] = np.array([0.5]).view(np.uint64)[0]
    prop_calls = {"all": [1.25 + 5e-16, 1.25 + 2e-15, NAN, NAN, -0.0, 0.0, INF, INF, 5e-324],
                  "back": [NAN, NAN, 1.25],          # a NaN over the same NaN, then home: no event
                  "below": [1.25 + 5e-16, 1.25 - 5e-16]}
    rec_calls = {"all": [0.5 + 0.000999, 0.5 - 0.000999, 0.5 + 0.001, 0.5, 0.5 - 0.001, NAN, NAN, 0.25],
                 "back": [NAN, NAN, 0.5],
                 "below": [0.5 + 0.000999, 0.5 - 0.000999]}
    assert 1.25 + 5e-16 != 1.25 and abs((1.25 + 2e-15) - 1.25) > 1e-15
    m = kernel.world_from_workload(w)
    gh, gd = w["guid_head"], w["guid_data"]
    expect_p, expect_r = {}, {}
    for name, o in objs.items():
        reads, ev = replay(1.25, prop_calls[name], accepts_float)
        for v, cur in zip(prop_calls[name], reads):
            m.set_props([gh[o]], [gd[o]], [X], [bits(v)])
            got = int(m.get_props([gh[o]], [gd[o]], [X])[0])
            assert got == bits(cur), (name, v, hex(got), hex(bits(cur)))
        expect_p[o] = (reads[-1], ev)
        reads, ev = replay(0.5, rec_calls[name], accepts_record_float)
        for v, cur in zip(rec_calls[name], reads):
            m.set_records([gh[o]], [gd[o]], [0], [ROW], [COL], [bits(v)])
            got = int(m.get_records([gh[o]], [gd[o]], [0], [ROW], [COL])[0])
            assert got == bits(cur), (name, v, hex(got), hex(bits(cur)))
        expect_r[o] = (reads[-1], ev)
    # (the model itself: the first call is refused, the second accepted; NaN over NaN and inf over inf are
    # accepted and change no bit; 0.0 over -0.0 is refused, so -0.0 stays)
    assert [bits(v) for v in replay(1.25, prop_calls["all"], accepts_float)[0]] == \
        [bits(v) for v in (1.25, 1.25 + 2e-15, NAN, NAN, -0.0, -0.0, INF, INF, 5e-324)]
    assert expect_p[objs["all"]][1] == (bits(1.25), bits(5e-324)) and expect_p[objs["back"]][1] is None
    assert expect_p[objs["below"]][1] is None and expect_r[objs["all"]][1] == (bits(0.5), bits(0.25))
    assert expect_r[objs["back"]][1] is None and expect_r[objs["below"]][1] is None
    m.ExecuteCalls()
    r = m.read_tick()
    assert r["summary"]["device_error"] == 0
    x_dev, cells = m.read_prop(X).view(np.uint64), m.read_record(0)
    ev = {(int(o), int(p)): (int(a), int(b)) for o, p, a, b in zip(r["ev_obj"], r["ev_pid"], r["ev_old"], r["ev_new"])}
    rrc = (0 << 16) | (ROW << 8) | COL
    re = {(int(o), int(c)): (int(a), int(b)) for o, c, a, b in zip(r["re_obj"], r["re_rrc"], r["re_old"], r["re_new"])}
    for o in objs.values():
        assert int(x_dev[o]) == bits(expect_p[o][0]) and ev.get((o, X)) == expect_p[o][1], o
        assert int(cells[o, COL, ROW]) == bits(expect_r[o][0]) and re.get((o, rrc)) == expect_r[o][1], o
        # and a Get after the frame reads the device's value
        assert int(m.get_props([gh[o]], [gd[o]], [X])[0]) == bits(expect_p[o][0])
    assert len(ev) == 1 and len(re) == 1
    m.close()
