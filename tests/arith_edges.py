"""Worlds that put the f64 / int64 effect arithmetic and the two Set predicates at their edges (a helper
module of tests/test_arith_edges.py, tests/test_gpu_arith_edges.py and tests/golden/gen_arith_golden.py;
no tests in it).

Every float a workload.make_world world feeds through the effect ops is a uniform random number of
magnitude >= 1 and every float constant of its programs is a power of two times a small integer, so a
fused multiply-add gives the bits a separate multiply and add gives, no Set lands near a predicate's
threshold, and no NaN, infinity, -0.0 or denormal passes anywhere.  The builders here take a make_world
dict and replace arrays in it: the programs (non-dyadic constants, constants a compiler folds, int64
extremes), the creation-time values, the SetProperty / SetRecordFloat call values, the f64 record cells.
Each is deterministic from its seed, 600-800 objects (three 256-slot tiles, the last one ragged) and at
most 10 frames.

Every property world's program working set fits k_tick's register slots (at most 12 destinations, 16
properties: nfgpu_device.hpp kMaxW / kMaxU), so the hipRTC kernel, the library kernel and k_tick_touch
all run it."""
import struct

import numpy as np

from noahgameframe_amd import workload as wl
from noahgameframe_amd.workload import (A_PROP, GUARD, GUARD_EQ0, GUARD_GT0, GUARD_LE0, GUARD_NE0, HI_PROP, I64_MAX,
                                        I64_MIN, KID, LO_PROP, N_INT, OP_FAFFINE, OP_FLERP, OP_FSET, OP_IADD_CLAMP,
                                        OP_ISET, OP_RFAFFINE, OP_RIADD_CLAMP, PID, guard)
from noahgameframe_amd.workload import f64bits as fb

# The one NaN of these worlds: x86-64's "real indefinite", the quiet NaN with the sign set that the
# reference's SSE2 code makes of inf - inf or inf * 0.  An operation with one NaN operand returns that
# operand, so with a single pattern every NaN of a run has these bits, whichever way it came.  Two NaNs of
# different bits in one add cannot be pinned: x86 keeps the instruction's first source, and which operand of
# the reference's `x + m` that is was the choice of its compiler's register allocation (this build's keeps
# m; the device's nan_of follows it), not of its source.  So the positive quiet NaN stays out of the lists.
NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
INF = float("inf")
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
DENORM = 5e-324
EPS_UP = float(np.nextafter(1e-15, 1.0))   # the first double NFCProperty::SetFloat's IsZeroDouble lets through

# Creation-time floats.  The reference harness loads them through NFCProperty::SetFloat, which on a
# still-null property refuses any |v| <= 1e-15 (PR:302-308): the property stays null and reads 0.0, while
# the oracle and the device hold the value from frame 0 on.  That is an artefact of loading, not of the
# path under test, so a creation-time float is exactly 0.0 or farther than 1e-15 from 0; tiny values, -0.0
# and denormals enter through SetProperty calls and program results only.
INIT_F_EDGES = [NAN, INF, -INF, DBL_MAX, -DBL_MAX, 1e300, 0.001, -0.001, EPS_UP, -EPS_UP, 3e-15, 0.0]
assert all(v == 0.0 or not abs(v) <= 1e-15 for v in INIT_F_EDGES)
# SetProperty call values: the above, and what may only enter after loading.
SET_F_EDGES = INIT_F_EDGES + [-0.0, DENORM, -DENORM, DBL_MIN, 1e-16, -1e-16]

# int64 values a 32-bit compare or add gets wrong
INT_EDGES = [1 << 32, (1 << 32) + 1, -(1 << 32) - 1, I64_MIN, I64_MAX, 0, 1, -1]

# f64 record cells.  NFCRecord's TData::operator== (NFIDataList.h:106-113) calls |d| < 0.001 equal.  Under
# RFAFFINE (0.9, 0.0007) a cell x moves by 0.0007 - 0.1 x: refused for x in (-0.003, 0.017) — so 0.0069,
# 0.007 (the fixed point), 0.0071, 0.011, +-0.001, -0.0 and 5e-324 are refused with a difference that is
# not 0 — and |d| sits at 0.001 (1 +- eps) for x next to 0.017 and -0.003.
REC_F_EDGES = [NAN, INF, -INF, -0.0, DENORM, 0.0069, 0.007, 0.0071, 0.011, 0.001, -0.001, 1e300, -1e300, DBL_MAX,
               0.017, float(np.nextafter(0.017, 1.0)), float(np.nextafter(0.017, 0.0)), 0.0169999, 0.0170001, 0.02,
               -0.003, float(np.nextafter(-0.003, -1.0)), float(np.nextafter(-0.003, 0.0)), -0.0030001, -0.0029999,
               -0.01]
RFAFFINE_AB = (0.9, 0.0007)

P = PID
FULL = (I64_MIN, I64_MAX)


def _bits(values):
    return np.array(values, np.float64).view(np.uint64)


# ---- programs ---------------------------------------------------------------------------------
# float_props: non-dyadic factors and pairs (a product by one is inexact, so a fused multiply-add rounds
# once where the reference rounds twice)
MOVE_F = [(OP_FLERP, 0, P["X"], 0, P["TargetX"], fb(0.1), 0),
          (OP_FLERP, 0, P["Y"], 0, P["TargetY"], fb(0.3), 0),
          (OP_FSET, A_PROP | GUARD, P["Z"], guard(P["Camp"], GUARD_GT0), P["TargetX"], 0, 0)]
PATROL_F = [(OP_FAFFINE, 0, P["TargetX"], 0, fb(-0.9), fb(1.0 / 3.0), 0),
            (OP_FAFFINE, 0, P["TargetY"], 0, fb(1.1), fb(0.3), 0),
            (OP_FSET, GUARD, P["AtkDis"], guard(P["Camp"], GUARD_EQ0), fb(2.7), 0, 0),
            (OP_FAFFINE, GUARD, P["AtkDis"], guard(P["Camp"], GUARD_GT0), fb(0.7), fb(0.1), 0)]


def _ntype(j):
    """an absorbing constant (0, NaN, inf, an assignment) runs on the objects of one NPCType only, so the
    other objects' values stay varied"""
    return guard(P["NPCType"], GUARD_EQ0, k=j)


# float_consts: the constants a compiler folds when it sees them as literals (the hipRTC kernel) and
# cannot when they come from a table (k_tick_dyn, k_tick_touch): x * 1.0, m + 0.0 (which turns -0.0 into
# +0.0), m + -0.0, x * 0.0 (-0.0 for a negative x, NaN for an infinite one), NaN and inf factors, a
# denormal addend; assignments of -0.0, NaN, inf and a denormal; lerps by 0.0, 1.0 and NaN
CONSTS = {
    "HPRegen": [(OP_FAFFINE, 0, P["Z"], 0, fb(1.0), fb(0.0), 0),
                (OP_FAFFINE, 0, P["Z"], 0, fb(1.0), fb(-0.0), 0),
                (OP_FAFFINE, 0, P["AtkDis"], 0, fb(-1.0), fb(-0.0), 0),
                (OP_FAFFINE, GUARD, P["Y"], _ntype(0), fb(0.0), fb(0.0), 0),
                (OP_FAFFINE, GUARD, P["Y"], _ntype(1), fb(NAN), fb(0.0), 0),
                (OP_FAFFINE, GUARD, P["Y"], _ntype(2), fb(INF), fb(0.0), 0),
                (OP_FAFFINE, 0, P["Z"], 0, fb(1.0), fb(DENORM), 0)],
    "MPRegen": [(OP_FLERP, GUARD, P["X"], _ntype(4), P["TargetX"], fb(0.0), 0),
                (OP_FLERP, 0, P["Z"], 0, P["TargetX"], fb(1.0), 0),
                (OP_FLERP, GUARD, P["X"], _ntype(5), P["TargetY"], fb(NAN), 0)],
    "Poison": [(OP_FSET, GUARD, P["TargetY"], _ntype(0), fb(-0.0), 0, 0),
               (OP_FSET, GUARD, P["TargetY"], _ntype(1), fb(NAN), 0, 0),
               (OP_FSET, GUARD, P["TargetY"], _ntype(2), fb(INF), 0, 0),
               (OP_FSET, GUARD, P["TargetY"], _ntype(3), fb(2.5e-310), 0, 0)],
}
assert sum(len(v) for v in CONSTS.values()) == 14

# int_edges: 9 int properties.  EXP only moves by +5 and SP by -7 over the whole int64 range (a cell near
# I64_MAX / I64_MIN wraps, as the reference's NFINT64 sum does); MP takes I64_MIN; Level is clamped to
# [DEF_VALUE, ATK_VALUE], which hold INT_EDGES (lo > hi in many objects: the result is hi); HP to the
# constants [100, 50]; the ISETs store +-(2^32 + 1) and 2^63 - 1; the guards compare ATK_VALUE, DEF_VALUE
# and Gold — which hold 2^32, 2^32 + 1, -2^32 - 1 and I64_MIN — with 0, with a constant and with each
# other.  ATK_VALUE, DEF_VALUE and Camp are operands only: SetProperty calls alone change them.
INTS = {
    "Move": [(OP_IADD_CLAMP, 0, P["EXP"], 0, 5, *FULL),
             (OP_IADD_CLAMP, 0, P["SP"], 0, -7, *FULL)],
    "MPRegen": [(OP_IADD_CLAMP, 0, P["MP"], 0, I64_MIN, *FULL),
                (OP_IADD_CLAMP, A_PROP | LO_PROP | HI_PROP, P["Level"], 0, P["Camp"], P["DEF_VALUE"], P["ATK_VALUE"]),
                (OP_IADD_CLAMP, GUARD, P["HP"], guard(P["Camp"], GUARD_EQ0, k=1), 1, 100, 50)],
    "Poison": [(OP_ISET, GUARD, P["HP"], guard(P["ATK_VALUE"], GUARD_NE0), (1 << 32) + 1, 0, 0),
               (OP_ISET, GUARD, P["Gold"], guard(P["ATK_VALUE"], GUARD_GT0, vs=P["DEF_VALUE"]), -(1 << 32) - 1, 0, 0),
               (OP_ISET, GUARD, P["Level"], guard(P["DEF_VALUE"], GUARD_EQ0, k=1), I64_MAX, 0, 0),
               (OP_IADD_CLAMP, GUARD, P["Gold"], guard(P["Gold"], GUARD_LE0, vs=P["ATK_VALUE"]), 1, -(1 << 40), 1 << 40)],
    "Patrol": [(OP_ISET, A_PROP | GUARD, P["MP"], guard(P["Gold"], GUARD_GT0), P["Gold"], 0, 0),
               (OP_IADD_CLAMP, A_PROP | GUARD, P["HP"], guard(P["DEF_VALUE"], GUARD_LE0, k=-1), P["ATK_VALUE"], *FULL)],
    "HPRegen": [(OP_IADD_CLAMP, A_PROP | HI_PROP, P["HP"], 0, P["DEF_VALUE"], 0, P["ATK_VALUE"])],
}
INT_PROPS_USED = ["EXP", "SP", "MP", "HP", "Gold", "Level", "ATK_VALUE", "DEF_VALUE", "Camp"]


def _set_programs(w, progs):
    """the kinds' programs replaced (a kind not named keeps one harmless op: a program is never empty)"""
    n_kind = int(w["cfg"][4])
    ops = np.zeros((n_kind, wl.MAX_OPS), wl.OP_DTYPE)
    n_ops = np.zeros(n_kind, np.int32)
    for k in range(n_kind):
        lst = progs.get(wl.KINDS[k], None)
        if lst is None:
            ops[k], n_ops[k] = w["ops"][k], w["n_ops"][k]
            continue
        assert 0 < len(lst) <= wl.MAX_OPS, (wl.KINDS[k], len(lst))
        for i, o in enumerate(lst):
            ops[k, i] = o
        n_ops[k] = len(lst)
    w["ops"], w["n_ops"] = ops, n_ops
    dst = {int(o["dst"]) for k in range(n_kind) for o in ops[k, :n_ops[k]] if o["code"] not in (OP_RIADD_CLAMP, OP_RFAFFINE)}
    assert len(dst) <= 12 and len(working_set(w)) <= 16, (len(dst), len(working_set(w)))


def working_set(w):
    """the properties the programs read or write"""
    s = set()
    for k in range(int(w["cfg"][4])):
        for o in w["ops"][k][:int(w["n_ops"][k])]:
            code, fl = int(o["code"]), int(o["flags"])
            if code in (OP_RIADD_CLAMP, OP_RFAFFINE):
                continue
            s.add(int(o["dst"]))
            if fl & GUARD:
                g = int(o["guard"])
                s.add(g & 0xFFFF)
                if g & wl.GUARD_PROP:
                    s.add(g >> 19)
            if code == OP_FLERP or ((fl & A_PROP) and code in (OP_IADD_CLAMP, OP_ISET, OP_FSET)):
                s.add(int(o["a"]))
            if code == OP_IADD_CLAMP and fl & LO_PROP:
                s.add(int(o["b"]))
            if code == OP_IADD_CLAMP and fl & HI_PROP:
                s.add(int(o["c"]))
    return s


# ---- values -----------------------------------------------------------------------------------
def _float_values(w, rng):
    """about 30 % of each float property's creation-time values from INIT_F_EDGES; about 20 % of the
    objects near the SetFloat threshold: X in [0.5, 2) and TargetX = X + j 2^-k, k in 48..53, j in
    -8..8 but 0, so that factor (TargetX - X) straddles 1e-15 where X's ulp is 2^-53 or 2^-52; about half of
    the float SetProperty values from SET_F_EDGES (make_world's duplicates — the same (object, property)
    twice in a window — stay)"""
    n = int(w["cfg"][0])
    f = np.array(w["init_f"], np.float64)
    edges = np.array(INIT_F_EDGES)
    for p in range(f.shape[0]):
        pick = rng.random(n) < 0.3
        f[p, pick] = rng.choice(edges, int(pick.sum()))
    near = rng.random(n) < 0.2
    m = int(near.sum())
    x = rng.uniform(0.5, 2.0, m)
    j = rng.integers(1, 9, m) * rng.choice([-1, 1], m)
    k = rng.integers(48, 54, m)
    f[P["X"] - N_INT, near] = x
    f[P["TargetX"] - N_INT, near] = x + j * np.exp2(-k.astype(np.float64))
    w["init_f"] = f
    xb = np.array(w["x_bits"], np.uint64)
    isf = np.asarray(w["x_pid"]) >= N_INT
    pick = isf & (rng.random(len(xb)) < 0.5)
    xb[pick] = _bits(rng.choice(np.array(SET_F_EDGES), int(pick.sum())))
    w["x_bits"] = xb


def near_threshold_objects(w):
    """the objects _float_values put next to the SetFloat threshold"""
    x, t = w["init_f"][P["X"] - N_INT], w["init_f"][P["TargetX"] - N_INT]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(t - x)
        return np.nonzero((x >= 0.5) & (x < 2.0) & (d > 0) & (d <= 8 * 2.0 ** -48))[0]


def _int_values(w, rng):
    """EXP within 5 of I64_MAX and SP within 7 of I64_MIN in a fifth of the objects each; Gold, ATK_VALUE,
    DEF_VALUE from INT_EDGES in half of them; half of the SetProperty values of the nine properties of
    INTS from INT_EDGES and the values next to the int64 ends"""
    n = int(w["cfg"][0])
    ii = np.array(w["init_i"], np.int64)
    edges = np.array(INT_EDGES, np.int64)
    hi = rng.random(n) < 0.2
    ii[P["EXP"], hi] = I64_MAX - rng.integers(0, 6, int(hi.sum()))
    lo = rng.random(n) < 0.2
    ii[P["SP"], lo] = I64_MIN + rng.integers(0, 8, int(lo.sum()))
    for name in ("Gold", "ATK_VALUE", "DEF_VALUE"):
        pick = rng.random(n) < 0.5
        ii[P[name], pick] = rng.choice(edges, int(pick.sum()))
    w["init_i"] = ii
    xb = np.array(w["x_bits"], np.uint64)
    used = np.isin(np.asarray(w["x_pid"]), [P[p] for p in INT_PROPS_USED])
    pick = used & (rng.random(len(xb)) < 0.5)
    vals = rng.choice(np.concatenate([edges, [I64_MAX - 2, I64_MIN + 3]]), int(pick.sum()))
    xb[pick] = vals.astype(np.int64).view(np.uint64)
    w["x_bits"] = xb


BASE = dict(n_scenes=2, groups_per_scene=4, players_per_group=3, host_ops=True)


# ---- builders ---------------------------------------------------------------------------------
def float_props(seed):
    """make_world's set_ops programs with every FLERP factor and FAFFINE pair non-dyadic, over edge values"""
    # (frames of 100 ms: Patrol, every 3 s, leaves two thirds of the objects' TargetX alone, so a Move
    # that the threshold refuses once is refused in every frame)
    w = wl.make_world(n_obj=700, n_ticks=10, seed=seed, tick_ms=100, set_ops=True, ext_props="all", ext_frac=0.3, **BASE)
    rng = np.random.default_rng(seed + 7001)
    patrol = [tuple(o) for o in w["ops"][KID["Patrol"]][:int(w["n_ops"][KID["Patrol"]])]]
    ints = [o for o in patrol if o[0] in (OP_IADD_CLAMP, OP_ISET)]
    assert len(ints) == 3 and ints[0][2] == P["Camp"]
    _set_programs(w, {"Move": MOVE_F, "Patrol": PATROL_F[:2] + ints[:1] + PATROL_F[2:] + ints[1:]})
    codes = w["ops"]["code"]
    assert not (codes == OP_RFAFFINE).any()
    _float_values(w, rng)
    return w


def float_consts(seed):
    w = wl.make_world(n_obj=650, n_ticks=10, seed=seed, tick_ms=500, ext_props="all", ext_frac=0.3, **BASE)
    rng = np.random.default_rng(seed + 7002)
    _set_programs(w, dict(CONSTS, Move=MOVE_F[:1], Patrol=PATROL_F[:1]))
    _float_values(w, rng)
    return w


def int_edges(seed):
    w = wl.make_world(n_obj=750, n_ticks=10, seed=seed, tick_ms=500, ext_frac=0.3,
                      ext_props=[P[p] for p in INT_PROPS_USED] + [P["X"], P["TargetX"]], **BASE)
    rng = np.random.default_rng(seed + 7003)
    _set_programs(w, INTS)
    _int_values(w, rng)
    return w


def arith(seed):
    """float_props' float ops, float_consts and int_edges in one world (the golden fixture `arith`)"""
    w = wl.make_world(n_obj=600, n_ticks=6, seed=seed, tick_ms=500, ext_props="all", ext_frac=0.25, **BASE)
    rng = np.random.default_rng(seed + 7004)
    progs = {"Move": MOVE_F, "Patrol": PATROL_F}
    for part in (CONSTS, INTS):
        for k, lst in part.items():
            progs[k] = progs.get(k, []) + lst
    _set_programs(w, progs)
    _float_values(w, rng)
    _int_values(w, rng)
    return w


def record_edges(seed):
    """RFAFFINE (0.9, 0.0007) over f64 cells from REC_F_EDGES; RIADD_CLAMP -100 over the whole int64 range on a
    cooldown column with cells next to I64_MIN (they wrap); SetRecordFloat values from the list, and the
    initial cell +- 0.000999... (refused) and +- 0.001 (accepted unless the sum rounds below it)"""
    w = wl.make_world(n_obj=640, n_scenes=2, groups_per_scene=3, players_per_group=40, n_ticks=10, seed=seed,
                      tick_ms=100, records=True, rec_rows=20, rec_set_float=True, rec_set_frac=0.1, rec_row_frac=0.05,
                      ext_frac=0.02, host_ops=True)
    rng = np.random.default_rng(seed + 7005)
    _set_programs(w, {"SkillCD": [(OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, -100, *FULL),
                                  (OP_RFAFFINE, 0, (0 << 8) | 2, 0, fb(RFAFFINE_AB[0]), fb(RFAFFINE_AB[1]), 0),
                                  (OP_RIADD_CLAMP, 0, (0 << 8) | 0, 0, 1, 1000, 1999)]})
    cells = np.array(w["rec0_cells"], np.uint64)
    n, _, rows = cells.shape
    pick = rng.random((n, rows)) < 0.4
    c2 = cells[:, 2, :]
    c2[pick] = _bits(rng.choice(np.array(REC_F_EDGES), int(pick.sum())))
    c1 = cells[:, 1, :].view(np.int64)
    low = rng.random((n, rows)) < 0.1
    c1[low] = I64_MIN + rng.integers(0, 300, int(low.sum()))
    w["rec0_cells"] = cells
    # the first window's calls once more before frame 0 (make_world's record calls start at frame 1, and no
    # heartbeat fires in frame 0: the AddSchedule calls made before it take effect at its end, SM:100-119),
    # so every frame has Update events on the f64 column
    first = np.asarray(w["r_tick"]) == 1
    for k in ("r_tick", "r_obj", "r_rec", "r_row", "r_col", "r_bits", "r_op", "r_vals"):
        head = np.zeros_like(w[k][first]) if k == "r_tick" else w[k][first]
        w[k] = np.concatenate([head, w[k]])
    # SetRecordFloat call values
    rb = np.array(w["r_bits"], np.uint64)
    isf = (np.asarray(w["r_col"]) == 2) & (np.asarray(w["r_op"]) == 0)
    idx = np.nonzero(isf)[0]
    cur = cells[w["r_obj"][idx], 2, w["r_row"][idx]].view(np.float64)
    r = rng.random(len(idx))
    sign = rng.choice([-1.0, 1.0], len(idx))
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(r < 0.4, rng.choice(np.array(REC_F_EDGES), len(idx)),
                     np.where(r < 0.55, cur + sign * 0.000999999999,
                              np.where(r < 0.7, cur + sign * 0.001, rb[idx].view(np.float64))))
    rb[idx] = v.view(np.uint64)
    w["r_bits"] = rb
    return w


BUILDERS = {"float_props": float_props, "float_consts": float_consts, "int_edges": int_edges,
            "record_edges": record_edges}
ARITH_SEED = 1414
