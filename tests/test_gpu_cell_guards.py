"""GPU: guards on record cells (NFK_GUARD_CELL) on every runner of the tick.

The C oracle predates the flag, so expected values come from twin worlds (workload.make_world(cell_guards=
(case, twin)); tests/test_cell_guards.py holds the generator to its contract): twin A guards on mirror int
properties and is pinned on the oracle here; twin B, the same workload but for its guard words, guards on
the record cells the mirrors track and must give A's outputs bit for bit — every event, recipient list,
fired heartbeat and final value, nothing filtered."""
import os
import subprocess
import sys

import numpy as np
import pytest

from noahgameframe_amd import kernel, workload as wl
from tests.parity import ROOT, compare_runs, run_gpu, run_oracle

pytestmark = pytest.mark.gpu
N_TICKS, SEED = 10, 11
PATHS = ["k_tick", "k_tick_dyn", "k_tick_touch"]
CASES = ["static", "replay", "unused_row_fixed_point", "calls"]


def set_path(monkeypatch, path):
    monkeypatch.setenv("NFGPU_ABLATE", "8" if path == "k_tick_touch" else "0")
    monkeypatch.setenv("NFGPU_JIT", "0" if path == "k_tick_dyn" else "1")


@pytest.fixture(scope="module")
def twins():
    """per case: twin A, twin B and the oracle's run of A, computed once and left unchanged"""
    cache = {}

    def get(case):
        if case not in cache:
            a = wl.make_world(cell_guards=(case, "A"), n_ticks=N_TICKS, seed=SEED)
            b = wl.make_world(cell_guards=(case, "B"), n_ticks=N_TICKS, seed=SEED)
            cache[case] = (a, b, run_oracle(a))
        return cache[case]
    return get


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES)
def test_cell_guard_twin_matches_mirror_twin(gpu_available, monkeypatch, twins, case, path):
    set_path(monkeypatch, path)
    a, b, ref = twins(case)
    if path == "k_tick":
        m = kernel.world_from_workload(b)
        on, msg = m.jit_status()
        m.close()
        assert on, msg
    got_a = run_gpu(a)
    compare_runs(run_gpu(b), got_a)   # the cell guards read what the mirror guards read
    compare_runs(got_a, ref)          # ... and A is what the oracle computes


def test_cell_guard_validation(gpu_available):
    """nfk_define_kind rejects a malformed NFK_GUARD_CELL op with NFK_ERR_ARG and a message naming the
    fault; a world with the flag on a valid cell commits"""
    P = wl.PID

    def world():
        m = kernel.NFKernelModule(64, n_class=2, n_kind=2, n_rec=2)
        m.define_record(0, 20, 3, [0, 0, 1], [wl.PRIVATE, wl.PRIVATE])   # record 1 stays undefined
        m.create_objects([7], [1], [1], [1], [wl.CLS_NPC], [0])
        return m

    def op(code, flags, dst, gd, a=1, b=0, c=100):
        return np.array([(code, flags, dst, gd, a, b, c)], wl.OP_DTYPE)

    ok_guard = wl.guard_cell(0, 19, 1, wl.GUARD_LE0, k=30)
    bad = {
        "NFK_GUARD_CELL without NFK_GUARD": op(wl.OP_IADD_CLAMP, wl.GUARD_CELL, P["Gold"], 0),
        "a record op takes no guard": op(wl.OP_RIADD_CLAMP, wl.GUARD | wl.GUARD_CELL, (0 << 8) | 1, ok_guard),
        "undefined record": op(wl.OP_IADD_CLAMP, wl.GUARD | wl.GUARD_CELL, P["Gold"], wl.guard_cell(1, 0, 0, wl.GUARD_GT0)),
        "undefined record ": op(wl.OP_IADD_CLAMP, wl.GUARD | wl.GUARD_CELL, P["Gold"], wl.guard_cell(5, 0, 0, wl.GUARD_GT0)),
        "row 20 outside": op(wl.OP_IADD_CLAMP, wl.GUARD | wl.GUARD_CELL, P["Gold"], wl.guard_cell(0, 20, 1, wl.GUARD_GT0)),
        "column 3 outside": op(wl.OP_ISET, wl.GUARD | wl.GUARD_CELL, P["Gold"], wl.guard_cell(0, 0, 3, wl.GUARD_GT0)),
        "not an int column": op(wl.OP_ISET, wl.GUARD | wl.GUARD_CELL, P["Gold"], wl.guard_cell(0, 0, 2, wl.GUARD_GT0)),
        "bits 13..15": op(wl.OP_ISET, wl.GUARD | wl.GUARD_CELL, P["Gold"], ok_guard | 0x2000),
    }
    m = world()
    for what, ops in bad.items():
        with pytest.raises(kernel.NFKError) as e:
            m.define_kind(0, ops)
        assert e.value.code == -1 and what.strip() in str(e.value), (what, str(e.value))
    # a record op under a plain guard is refused as before
    with pytest.raises(kernel.NFKError) as e:
        m.define_kind(0, op(wl.OP_RIADD_CLAMP, wl.GUARD, (0 << 8) | 1, wl.guard(P["HP"], wl.GUARD_GT0)))
    assert e.value.code == -1
    # the shape is checked again at commit: the record redefined smaller after the kind
    m.define_kind(0, op(wl.OP_IADD_CLAMP, wl.GUARD | wl.GUARD_CELL, P["Gold"], ok_guard))
    m.define_kind(1, op(wl.OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, -100, 0, wl.I64_MAX))
    m.define_record(1, 4, 1, [0], [0, 0])
    m.define_record(0, 10, 3, [0, 0, 1], [wl.PRIVATE, wl.PRIVATE])
    with pytest.raises(kernel.NFKError) as e:
        m.commit()
    assert e.value.code == -1 and "row 19 outside" in str(e.value)
    m.close()
    m = world()
    m.define_record(1, 4, 1, [0], [0, 0])
    m.define_kind(0, op(wl.OP_IADD_CLAMP, wl.GUARD | wl.GUARD_CELL, P["Gold"], ok_guard))
    m.define_kind(1, op(wl.OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, -100, 0, wl.I64_MAX))
    m.commit()
    m.close()


@pytest.mark.parametrize("chain_u", ["1", "0"])
def test_cell_guard_chain_matches_mirror_twin(gpu_available, tmp_path, chain_u):
    """the per-Set log (nfk_watch_props / nfk_read_chain) of the `replay` case with the guarded ops'
    destinations watched: B's log equals A's, on k_chain_u (NFGPU_CHAIN_U=1) and on k_chain (=0).  The
    library reads NFGPU_CHAIN_U once per process, so each setting runs in a process of its own
    (tests/cell_guard_chain.py)."""
    out = str(tmp_path / "chain.npz")
    env = dict(os.environ, NFGPU_CHAIN_U=chain_u, NFGPU_JIT="1", NFGPU_ABLATE="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cell_guard_chain.py"), out, str(N_TICKS), str(SEED)],
                   check=True, env=env, cwd=ROOT)
    z = np.load(out)
    n = 0
    for t in range(N_TICKS):
        for k in ("obj", "kind", "op", "pid", "old", "new"):
            a, b = z[f"a_t{t}_{k}"], z[f"b_t{t}_{k}"]
            assert a.shape == b.shape and np.array_equal(a, b), (t, k)
        n += len(z[f"a_t{t}_obj"])
    assert n > 1000, n   # the guarded Sets are logged, frame after frame


def _chain_run(tmp_path, name, env, *watch):
    out = str(tmp_path / f"{name}.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cell_guard_chain.py"), out, str(N_TICKS), str(SEED), *watch],
                   check=True, env=dict(os.environ, NFGPU_JIT="1", NFGPU_ABLATE="0", **env), cwd=ROOT)
    z = np.load(out)
    return {tw: [tuple(z[f"{tw}_t{t}_{k}"].tolist() for k in ("obj", "kind", "op", "pid", "old", "new")) for t in range(N_TICKS)]
            for tw in ("a", "b")}


@pytest.mark.parametrize("chain_u", ["1", "0"])
def test_cell_guard_chain_closure_follows_record_columns(gpu_available, tmp_path, chain_u):
    """the `replay` case with only Gold watched: the kinds that write Gold (HPRegen, Patrol) are re-run, and
    Patrol's guard reads the column Move's RIADD_CLAMP writes; Move writes no watched property, and in twin
    B no property a re-run kind reads, so only the closure's record-column rule re-runs it.  B's log equals
    A's (whose Move enters through the mirror it writes); without the closure (NFGPU_CHAIN_NO_CLOSURE=1)
    B's Patrol guards read the cell before Move's op and the log differs."""
    ref = _chain_run(tmp_path, "closure", dict(NFGPU_CHAIN_U=chain_u), "Gold")
    assert ref["b"] == ref["a"]
    n = sum(len(f[0]) for f in ref["a"])
    assert n > 1000, n
    gold = {p for f in ref["a"] for p in f[3]}
    assert gold == {wl.PID["Gold"]}
    bare = _chain_run(tmp_path, "no_closure", dict(NFGPU_CHAIN_U=chain_u, NFGPU_CHAIN_NO_CLOSURE="1"), "Gold")
    assert bare["b"] != ref["a"]


ADAPTER_EXE = os.path.join(ROOT, "oracle", "_ref", "adapter_session")


def test_cell_guard_twins_through_the_plugin(gpu_available, tmp_path):
    """the plugin layer: twins A and B of the `static` case (reduced to 1200 objects in 2 x 3 groups, 6
    frames) written with nfio.write and replayed through tests/cpp/adapter_session.cpp — the reference's
    kernel and class modules over the adapter, which registers every program BY NAME
    (NFGPUKernelModule::AddHeartBeatProgram(name, ops, props, records): the guard cell's record is resolved
    through `records` at AfterInit, the flag passed through).  The two output files hold the same arrays,
    and they are A's oracle outputs where the session's are comparable as they stand (the final
    properties)."""
    from noahgameframe_amd import nfio
    if not os.path.exists(ADAPTER_EXE):
        pytest.skip("adapter_session not built (needs the reference's sources at build time)")
    over = dict(n_obj=1200, n_scenes=2, groups_per_scene=3)
    outs = {}
    for tw in ("A", "B"):
        w = wl.make_world(cell_guards=("static", tw, over), n_ticks=6, seed=SEED)
        wp, op = str(tmp_path / f"w{tw}.nfio"), str(tmp_path / f"o{tw}.nfio")
        nfio.write(wp, w)
        subprocess.run([ADAPTER_EXE, wp, op], check=True, timeout=300)
        outs[tw] = nfio.read(op)
        if tw == "A":
            ref = run_oracle(w)
    a, b = outs["A"], outs["B"]
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k]), k
    assert sum(len(a[f"ev_t{t}_obj"]) for t in range(6)) > 1000
    np.testing.assert_array_equal(a["final_i"], ref["final_i"])
