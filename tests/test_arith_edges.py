"""CPU: the edge worlds of tests/arith_edges.py.  The oracle equals the compiled reference on them; they do
reach the edges they are built for (checked on the oracle's output); and an oracle built with fused
multiply-adds — the mutation a build line that lost -ffp-contract=off would be — differs on them, while it
is identical on the older fixtures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from noahgameframe_amd import nfio, workload as wl
from tests import arith_edges
from tests.parity import REF, ROOT, _run_cli, compare_runs, run_oracle, run_ref

GOLDEN = os.path.join(ROOT, "tests", "golden")
have_ref = os.path.exists(REF)
P = wl.PID
I64 = np.iinfo(np.int64)

_runs = {}


def oracle_run(name, seed=1):
    """a builder's world and the oracle's run of it, computed once and shared (never changed)"""
    if (name, seed) not in _runs:
        w = arith_edges.BUILDERS[name](seed)
        _runs[name, seed] = (w, run_oracle(w))
    return _runs[name, seed]


@pytest.mark.skipif(not have_ref, reason="oracle/_ref not built (needs the reference's sources)")
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", ["float_props", "float_consts", "int_edges"])
def test_oracle_matches_reference_on_edge_worlds(name, seed):
    """the compiled NFCProperty::SetInt / SetFloat (PR:254, PR:295) under the same programs and calls"""
    w, o = oracle_run(name, seed)
    compare_runs(o, run_ref(w))


def test_builders_are_deterministic_and_fit_the_register_slots():
    for name, build in arith_edges.BUILDERS.items():
        a, b = build(5), build(5)
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), (name, k)
        assert 600 <= int(a["cfg"][0]) <= 800 and int(a["cfg"][7]) <= 10
        assert len(arith_edges.working_set(a)) <= 16
    w = arith_edges.arith(arith_edges.ARITH_SEED)
    g = nfio.read(os.path.join(GOLDEN, "arith.workload.nfio"))
    assert sorted(w) == sorted(g)
    for k in w:   # the committed fixture is the builder's world
        assert np.array_equal(np.ascontiguousarray(w[k]).view(np.uint8).ravel(),
                              np.ascontiguousarray(g[k]).view(np.uint8).ravel()), k


def test_initial_floats_load_through_the_reference():
    """a creation-time float within 1e-15 of 0 but not 0 would stay null in the reference (PR:302-308)"""
    for name in ("float_props", "float_consts"):
        f = oracle_run(name)[0]["init_f"]
        assert not ((f != 0) & (np.abs(f) <= 1e-15)).any()
        assert not ((f == 0) & np.signbit(f)).any()


def test_float_props_reaches_the_setfloat_threshold():
    w, o = oracle_run("float_props")
    near = arith_edges.near_threshold_objects(w)
    xi = P["X"] - wl.N_INT
    same = o["final_f"][xi][near].view(np.uint64) == w["init_f"][xi][near].view(np.uint64)
    print("near-threshold objects", len(near), "X unchanged", int(same.sum()), "changed", int((~same).sum()))
    assert same.sum() >= 20 and (~same).sum() >= 20
    # the accepted Moves of these objects (one a frame; frames with a SetProperty call on X aside) include
    # steps of a few ulps: differences between 1e-15 and 1e-14
    small = 0
    for t in range(int(w["cfg"][7])):
        called = np.asarray(w["x_obj"])[(np.asarray(w["x_tick"]) == t) & (np.asarray(w["x_pid"]) == P["X"])]
        sel = (o[f"ev_t{t}_pid"] == P["X"]) & np.isin(o[f"ev_t{t}_obj"], near) & ~np.isin(o[f"ev_t{t}_obj"], called)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(o[f"ev_t{t}_new"][sel].view(np.float64) - o[f"ev_t{t}_old"][sel].view(np.float64))
        assert not (d <= 1e-15).any()
        small += int((d < 1e-14).sum())
    assert small >= 20, small
    f = np.asarray(o["final_f"])
    n_nan, n_inf, n_negz = int(np.isnan(f).sum()), int(np.isinf(f).sum()), int(((f == 0) & np.signbit(f)).sum())
    print("final NaN", n_nan, "inf", n_inf, "-0.0", n_negz)
    assert n_nan >= 10 and n_inf >= 10 and n_negz >= 1
    # a window sets the same (object, property) twice
    pairs = np.stack([w["x_tick"], w["x_obj"], w["x_pid"]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)


def test_float_consts_reaches_signed_zeros_and_made_nans():
    w, o = oracle_run("float_consts")
    f = np.asarray(o["final_f"])
    assert ((f == 0) & np.signbit(f)).sum() >= 10 and ((f == 0) & ~np.signbit(f)).sum() >= 10
    assert np.isnan(f).sum() >= 10 and np.isinf(f).sum() >= 10
    assert ((f != 0) & (np.abs(f) < np.finfo(np.float64).tiny)).sum() >= 10   # denormals
    # every NaN, set or made by an op (inf * 0, inf - inf), has the one pattern of these worlds
    assert (f.view(np.uint64)[np.isnan(f)] == 0xFFF8000000000000).all()
    # and ops did make some: more NaNs in Y than the values and calls put there and NaN * x spreads
    y = wl.PID["Y"] - wl.N_INT
    made = np.isnan(f[y]) & ~np.isnan(w["init_f"][y]) & np.isin(w["init_i"][wl.PID["NPCType"]], [0, 2])
    assert made.sum() >= 10   # 0.0 * inf and inf * +-0.0 under the NPCType 0 and 2 guards


def record_f64_model(w, o):
    """Column 2 of record 0 replayed in numpy (a multiply, then an add: two roundings) for the objects
    without row operations: per frame the window's SetRecordFloat calls on used rows, then RFAFFINE on
    every used row of the objects whose SkillCD fired.  Returns (objects, their cells at the end, Sets
    refused with a difference that is not 0, Sets accepted with |d| < 0.002)."""
    a, b = arith_edges.RFAFFINE_AB
    n, _, rows = w["rec0_cells"].shape
    keep = np.ones(n, bool)
    keep[np.asarray(w["r_obj"])[np.asarray(w["r_op"]) != 0]] = False
    c = np.array(w["rec0_cells"][:, 2, :]).view(np.float64).copy()
    used = ((np.asarray(w["rec0_used"])[:, None] >> np.arange(rows, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    refused = accepted = 0

    def put(cur, v):
        nonlocal refused, accepted
        with np.errstate(invalid="ignore", over="ignore"):
            d = v - cur
            eq = (d < 0.001) & (d > -0.001)
            refused += int((eq & (d != 0)).sum())
            accepted += int((~eq & (np.abs(d) < 0.002)).sum())
        return np.where(eq, cur, v)

    for t in range(int(w["cfg"][7])):
        for i in np.nonzero((np.asarray(w["r_tick"]) == t) & (np.asarray(w["r_op"]) == 0) & (np.asarray(w["r_col"]) == 2))[0]:
            ob, row = int(w["r_obj"][i]), int(w["r_row"][i])
            if keep[ob] and used[ob, row]:
                c[ob, row] = put(c[ob, row:row + 1], np.asarray(w["r_bits"][i:i + 1]).view(np.float64))[0]
        fired = np.zeros(n, bool)
        fired[o[f"fi_t{t}_obj"][o[f"fi_t{t}_kind"] == wl.KID["SkillCD"]]] = True
        m = (fired & keep)[:, None] & used
        with np.errstate(invalid="ignore", over="ignore"):
            v = c[m] * a
            v = v + b
        c[m] = put(c[m], v)
    return np.nonzero(keep)[0], c[keep], refused, accepted


def test_record_edges_reaches_the_record_threshold():
    w, o = oracle_run("record_edges")
    for t in range(int(w["cfg"][7])):
        rrc = o[f"re_t{t}_rrc"]
        assert (((rrc >> 24) == 0) & ((rrc & 0xFF) == 2)).any(), f"frame {t}: no Update event on the f64 column"
    objs, cells, refused, accepted = record_f64_model(w, o)
    print("objects replayed", len(objs), "refused with d != 0", refused, "accepted with |d| < 0.002", accepted)
    assert len(objs) > 300 and refused >= 20 and accepted >= 20
    assert np.array_equal(cells.view(np.uint64), o["final_rec0"][objs, 2, :])
    # the cooldown column wraps: an Update from next to I64_MIN to next to I64_MAX
    wraps = 0
    for t in range(int(w["cfg"][7])):
        sel = ((o[f"re_t{t}_rrc"] >> 24) == 0) & ((o[f"re_t{t}_rrc"] & 0xFF) == 1)
        old, new = o[f"re_t{t}_old"][sel].view(np.int64), o[f"re_t{t}_new"][sel].view(np.int64)
        wraps += int(((old < I64.min + 400) & (new > I64.max - 400)).sum())
    assert wraps >= 20, wraps


def test_int_edges_reaches_wraps_inverted_clamps_and_wide_guards():
    w, o = oracle_run("int_edges")
    nt, n = int(w["cfg"][7]), int(w["cfg"][0])
    ii = w["init_i"]
    set_pids = {p: set(np.asarray(w["x_obj"])[np.asarray(w["x_pid"]) == P[p]].tolist()) for p in arith_edges.INT_PROPS_USED}
    quiet = lambda *props: np.array([all(ob not in set_pids[p] for p in props) for ob in range(n)])   # noqa: E731
    fired = {k: np.zeros(n, bool) for k in wl.KINDS[:5]}
    up = down = inverted = 0
    for t in range(nt):
        for k in fired:
            fired[k][o[f"fi_t{t}_obj"][o[f"fi_t{t}_kind"] == wl.KID[k]]] = True
        ob, pid = o[f"ev_t{t}_obj"], o[f"ev_t{t}_pid"]
        old, new = o[f"ev_t{t}_old"].view(np.int64), o[f"ev_t{t}_new"].view(np.int64)
        # EXP only ever takes +5 and SP -7 over the whole range: a step the other way is a wrap
        q = quiet("EXP")[ob]
        down += int(((pid == P["EXP"]) & q & (new < old)).sum())
        q = quiet("SP")[ob]
        up += int(((pid == P["SP"]) & q & (new > old)).sum())
        # Level clamped to [DEF_VALUE, ATK_VALUE] with lo > hi lands on hi
        q = quiet("Level", "ATK_VALUE", "DEF_VALUE", "Camp")[ob] & (ii[P["DEF_VALUE"]][ob] > ii[P["ATK_VALUE"]][ob])
        inverted += int(((pid == P["Level"]) & q & (new == ii[P["ATK_VALUE"]][ob])).sum())
    print("wraps past I64_MAX", down, "past I64_MIN", up, "clamps with lo > hi", inverted)
    assert down >= 1 and up >= 1 and inverted >= 1
    # the constant form: HP + 1 clamped to [100, 50] ran on the objects of Camp 1 whose MPRegen fired
    assert (fired["MPRegen"] & quiet("Camp") & (ii[P["Camp"]] == 1)).sum() >= 1
    # guards whose operands do not fit int32, where a compare of the low halves answers otherwise:
    # Poison's `ATK_VALUE != 0` (left side) and `ATK_VALUE > DEF_VALUE` (both sides)
    atk, dfv = ii[P["ATK_VALUE"]], ii[P["DEF_VALUE"]]
    wide = lambda v: (v > 2 ** 31 - 1) | (v < -2 ** 31)   # noqa: E731
    ran = fired["Poison"] & quiet("ATK_VALUE", "DEF_VALUE")
    lo32 = lambda v: v.astype(np.int32)   # noqa: E731  (the low half, as a 32-bit compare would read it)
    left = ran & wide(atk) & ((atk != 0) != (lo32(atk) != 0))
    both_l = ran & wide(atk) & ((atk > dfv) != (lo32(atk) > lo32(dfv)))
    both_r = ran & wide(dfv) & ((atk > dfv) != (lo32(atk) > lo32(dfv)))
    print("wide guard operands: left of != 0", int(left.sum()), "left of >", int(both_l.sum()), "right of >", int(both_r.sum()))
    assert left.sum() >= 1 and both_l.sum() >= 1 and both_r.sum() >= 1
    # and the constant form, `DEF_VALUE == 1` with DEF_VALUE = 2^32 + 1
    assert (ran & (dfv == (1 << 32) + 1)).sum() >= 1
    # SetProperty calls carry the same values
    xv = np.asarray(w["x_bits"]).view(np.int64)[np.asarray(w["x_pid"]) < wl.N_INT]
    assert wide(xv).sum() >= 50 and (xv == I64.min).any() and (xv == I64.max).any()


# ---- a build that contracts a multiply and an add ---------------------------------------------------
def _fma_oracle(tmp_path_factory):
    """oracle/nf_oracle.c with the Makefile's flags but -ffp-contract=fast -mfma; None when this machine
    cannot run fused multiply-adds or the compiler made none"""
    if "exe" not in _fma:
        _fma["exe"] = None
        try:
            flags = open("/proc/cpuinfo").read()
        except OSError:
            flags = ""
        if " fma" in flags and shutil.which("gcc") and shutil.which("objdump"):
            exe = str(tmp_path_factory.mktemp("fma") / "nf_oracle_fma")
            subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=fast", "-mfma", "-fno-fast-math", "-o", exe,
                            os.path.join(ROOT, "oracle", "nf_oracle.c"), "-lm"], check=True)
            asm = subprocess.run(["objdump", "-d", exe], check=True, capture_output=True, text=True).stdout
            if any(x in asm for x in ("vfmadd", "vfmsub", "vfnmadd", "vfnmsub")):
                _fma["exe"] = exe
    return _fma["exe"]


_fma = {}


def _differs(a, b):
    return [k for k in sorted(a) if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8).ravel(),
                                                       np.ascontiguousarray(b[k]).view(np.uint8).ravel())]


@pytest.mark.parametrize("name", ["float_props", "record_edges", "arith", "props"])
def test_worlds_see_a_contracted_build(tmp_path_factory, name):
    """The device library, the hipRTC options and the oracle are all built with -ffp-contract=off.  An
    oracle that fuses x * a + b differs from the normal one on float_props, record_edges and the `arith`
    golden workload — these worlds would fail a build line that lost the flag — and is IDENTICAL on the
    golden `props` workload, whose constants are all dyadic (the gap these worlds close)."""
    exe = _fma_oracle(tmp_path_factory)
    if exe is None:
        pytest.skip("no fma on this machine, or the compiler fused nothing")
    if name in arith_edges.BUILDERS:
        w, normal = oracle_run(name)
    else:
        w = nfio.read(os.path.join(GOLDEN, f"{name}.workload.nfio"))
        normal = run_oracle(w)
    diff = _differs(normal, _run_cli(exe, w))
    if name == "props":
        assert diff == []
    else:
        assert diff, "a fused multiply-add changes nothing in this world"
        assert any(k.startswith("ev_t") or k.startswith("re_t") for k in diff) and any(k.startswith("final_") for k in diff)
