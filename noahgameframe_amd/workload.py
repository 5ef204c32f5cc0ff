"""Synthetic NoahGameFrame worlds (product-side input generation, no oracle code).

A world mirrors the reference's game-server shape: NPC / Player classes whose
property flags follow _Out/NFDataCfg/Struct/Class/{IObject,NPC,Player}.xml,
objects grouped into (scene, group) cells (NFCSceneInfo / NFCSceneGroupInfo),
heartbeats registered through NFIScheduleModule::AddSchedule with effect
programs, optional per-player records (item/skill tables with cooldowns),
SetProperty calls from game logic between frames, and AddSchedule /
RemoveSchedule calls between frames.

`make_world(...)` returns a dict of numpy arrays in the NFIO layout consumed by
the GPU path (noahgameframe_amd.kernel), the CPU oracle and the reference
harness.
"""
import struct

import numpy as np

# ---- schema ---------------------------------------------------------------
INT_PROPS = ["HP", "MAXHP", "HPREGEN", "MP", "MAXMP", "MPREGEN", "SP", "MAXSP",
             "SPREGEN", "EXP", "Gold", "Level", "ATK_VALUE", "DEF_VALUE", "Camp", "NPCType",
             "SceneID", "GroupID"]
FLT_PROPS = ["X", "Y", "Z", "TargetX", "TargetY", "AtkDis"]
PROPS = INT_PROPS + FLT_PROPS
PID = {n: i for i, n in enumerate(PROPS)}
N_INT, N_FLT = len(INT_PROPS), len(FLT_PROPS)

# object (NFGUID) properties, TDATA_OBJECT (NFIDataList.h): prop ids after the int and float ones
# (a world has them with make_world(obj_props=True))
OBJ_PROPS = ["LastAttacker", "MasterID", "TargetID"]

PUBLIC, PRIVATE, UPLOAD = 1, 2, 4
CLS_NPC, CLS_PLAYER = 0, 1

# heartbeat kinds: id order == lexical order of the schedule names (NFMapEx<std::string, ...>)
KINDS = ["HPRegen", "MPRegen", "Move", "Patrol", "Poison", "SkillCD"]
assert KINDS == sorted(KINDS)
KID = {n: i for i, n in enumerate(KINDS)}

# op codes / flags (include/nfgpu.h)
OP_IADD_CLAMP, OP_FLERP, OP_FAFFINE, OP_RIADD_CLAMP, OP_RFAFFINE, OP_ISET, OP_FSET = 1, 2, 3, 4, 5, 6, 7
A_PROP, LO_PROP, HI_PROP, GUARD = 1, 2, 4, 8
GUARD_CELL = 16
GUARD_GT0, GUARD_LE0, GUARD_NE0, GUARD_EQ0 = 0, 1, 2, 3
GUARD_PROP = 1 << 18
GUARD_KMIN, GUARD_KMAX = -4096, 4095


def guard(pid, cmp, vs=None, k=0):
    """nfk_op.guard of an NFK_GUARD op: the int property and its comparison with the constant k (0 by
    default; NFK_GUARD_K, a functor's `if (GetPropertyInt(self, g) > 30)`), or with the int property
    `vs` (NFK_GUARD_PROP: a functor's `if (GetPropertyInt(self, g) > GetPropertyInt(self, h))`)"""
    assert GUARD_KMIN <= k <= GUARD_KMAX and (vs is None or k == 0)
    return pid | (cmp << 16) | ((k & 0x1FFF) << 19 if vs is None else GUARD_PROP | (vs << 19))


def guard_cell(rec, row, col, cmp, vs=None, k=0):
    """nfk_op.guard of an NFK_GUARD | NFK_GUARD_CELL op: the int record cell (NFK_GUARD_CELL_ID: rec << 10 |
    row << 4 | col) and its comparison with the constant k or the int property `vs`, as guard() — a
    functor's `if (GetRecordInt(self, rec, row, col) <= 0)`"""
    assert 0 <= rec < 8 and 0 <= row < 64 and 0 <= col < 16
    return guard((rec << 10) | (row << 4) | col, cmp, vs, k)


MAX_OPS = 8  # include/nfgpu.h NFK_MAX_OPS (workload files written before round 4 hold 4 per kind)
MAX_REC_COLS = 16
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1

OP_DTYPE = np.dtype([("code", "u1"), ("flags", "u1"), ("dst", "<u2"), ("guard", "<u4"),
                     ("a", "<i8"), ("b", "<i8"), ("c", "<i8")])
assert OP_DTYPE.itemsize == 32


def f64bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _prop_flags(n_oprops=0):
    f = np.zeros((2, len(PROPS) + n_oprops), np.uint8)
    pubpriv = PUBLIC | PRIVATE
    for c in (CLS_NPC, CLS_PLAYER):
        for n in ["HP", "MAXHP", "HPREGEN", "MP", "MAXMP", "MPREGEN", "SP", "MAXSP", "SPREGEN",
                  "EXP", "Gold", "Level", "ATK_VALUE", "DEF_VALUE", "X", "Y", "Z"]:
            f[c, PID[n]] = pubpriv
    f[CLS_NPC, PID["Camp"]] = PRIVATE             # NPC.xml: Camp Public=0 Private=1
    f[CLS_PLAYER, PID["Camp"]] = pubpriv          # Player.xml: Camp Public=1 Private=1
    f[CLS_PLAYER, PID["Gold"]] = PRIVATE | UPLOAD  # an Upload property never echoes to its owner
    # IObject.xml: SceneID / GroupID Public=0 Private=1
    for c in (CLS_NPC, CLS_PLAYER):
        f[c, PID["SceneID"]] = PRIVATE
        f[c, PID["GroupID"]] = PRIVATE
    # NPCType, TargetX, TargetY, AtkDis: Public=0 Private=0 (no sync)
    if n_oprops:  # LastAttacker public, MasterID private, TargetID private & upload (to nobody)
        base = len(PROPS)
        for c in (CLS_NPC, CLS_PLAYER):
            f[c, base + 0] = PUBLIC | PRIVATE
            f[c, base + 1] = PRIVATE
            f[c, base + 2] = PRIVATE | UPLOAD
    return f


def programs(with_records, rec_float_op=True, rec_skill_op=False, set_ops=False, lethal_poison=False,
             const_guards=False):
    ops = np.zeros((len(KINDS), MAX_OPS), OP_DTYPE)
    n_ops = np.zeros(len(KINDS), np.int32)

    def put(kind, lst):
        for i, o in enumerate(lst):
            ops[KID[kind], i] = o
        n_ops[KID[kind]] = len(lst)

    put("HPRegen", [(OP_IADD_CLAMP, A_PROP | HI_PROP, PID["HP"], 0, PID["HPREGEN"], 0, PID["MAXHP"])])
    put("MPRegen", [(OP_IADD_CLAMP, A_PROP | HI_PROP, PID["MP"], 0, PID["MPREGEN"], 0, PID["MAXMP"])])
    put("Move", [(OP_FLERP, 0, PID["X"], 0, PID["TargetX"], f64bits(0.125), 0),
                 (OP_FLERP, 0, PID["Y"], 0, PID["TargetY"], f64bits(0.125), 0)])
    put("Patrol", [(OP_FAFFINE, 0, PID["TargetX"], 0, f64bits(-1.0), f64bits(0.0), 0),
                   (OP_FAFFINE, 0, PID["TargetY"], 0, f64bits(-1.0), f64bits(0.0), 0)])
    put("Poison", [(OP_IADD_CLAMP, HI_PROP, PID["HP"], 0, -13, 1, PID["MAXHP"])])
    if set_ops:
        # plain assignments a functor makes (SetPropertyInt / SetPropertyFloat with a constant or
        # another property's value): first Sets change the value, repeated ones raise no event; some
        # under a guard on an int property (a functor's `if (GetPropertyInt(self, g) ...)`), one of
        # them on a value the same program wrote just before
        # (round 5: guards comparing two int properties, NFK_GUARD_PROP, in MPRegen, Patrol and Poison)
        put("MPRegen", [(OP_IADD_CLAMP, A_PROP | HI_PROP, PID["MP"], 0, PID["MPREGEN"], 0, PID["MAXMP"]),
                        (OP_ISET, A_PROP | GUARD, PID["EXP"], guard(PID["Camp"], GUARD_NE0), PID["Level"], 0, 0),
                        (OP_IADD_CLAMP, HI_PROP | GUARD, PID["MP"], guard(PID["MP"], GUARD_GT0, vs=PID["SP"]), -3, 0,
                         PID["MAXMP"])])
        put("Move", [(OP_FLERP, 0, PID["X"], 0, PID["TargetX"], f64bits(0.125), 0),
                     (OP_FLERP, 0, PID["Y"], 0, PID["TargetY"], f64bits(0.125), 0),
                     (OP_FSET, A_PROP | GUARD, PID["Z"], guard(PID["Camp"], GUARD_GT0), PID["TargetX"], 0, 0)])
        put("Patrol", [(OP_FAFFINE, 0, PID["TargetX"], 0, f64bits(-1.0), f64bits(0.0), 0),
                       (OP_FAFFINE, 0, PID["TargetY"], 0, f64bits(-1.0), f64bits(0.0), 0),
                       (OP_IADD_CLAMP, 0, PID["Camp"], 0, -1, 0, 3),
                       (OP_FSET, GUARD, PID["AtkDis"], guard(PID["Camp"], GUARD_EQ0), f64bits(2.5), 0, 0),
                       (OP_FAFFINE, GUARD, PID["AtkDis"], guard(PID["Camp"], GUARD_GT0), f64bits(1.5), f64bits(0.25), 0),
                       (OP_IADD_CLAMP, A_PROP, PID["SP"], 0, PID["Level"], 0, 1000),  # (6 ops: > 4 per program)
                       (OP_ISET, A_PROP | GUARD, PID["SP"], guard(PID["Level"], GUARD_LE0, vs=PID["Camp"]), PID["Level"], 0, 0)])
        put("Poison", [(OP_IADD_CLAMP, HI_PROP, PID["HP"], 0, -13, 1, PID["MAXHP"]),
                       (OP_ISET, GUARD, PID["SP"], guard(PID["Camp"], GUARD_LE0), 7, 0, 0),
                       (OP_ISET, GUARD, PID["EXP"], guard(PID["HP"], GUARD_EQ0, vs=PID["MAXHP"]), 0, 0, 0),
                       (OP_IADD_CLAMP, GUARD, PID["EXP"], guard(PID["SP"], GUARD_NE0, vs=PID["Level"]), 1, 0, 1 << 40)])
    if lethal_poison:
        # Poison may kill: HP clamps at 0, and the same functor revives a dead object at 3 HP — within
        # one frame HP goes hp -> 0 -> 3, so NFCNPCRefreshModule::OnObjectHPEvent-style per-object
        # callbacks (newVar <= 0 kills, NFCNPCRefreshModule.cpp:113-116) see the death only when they
        # fire once per accepted Set
        put("Poison", [(OP_IADD_CLAMP, HI_PROP, PID["HP"], 0, -13, 0, PID["MAXHP"]),
                       (OP_ISET, GUARD, PID["HP"], guard(PID["HP"], GUARD_LE0), 3, 0, 0)])
    if const_guards:
        # guards against constants other than 0 (round 6, NFK_GUARD_K): a functor's
        # `if (GetPropertyInt(self, "Level") > 30)`; ATK_VALUE falls by 900 a Poison fire, so the guards
        # on it meet negative constants and both ends of the range (<= -4096 lifts it by 9000 to > 4095)
        put("HPRegen", [(OP_IADD_CLAMP, A_PROP | HI_PROP, PID["HP"], 0, PID["HPREGEN"], 0, PID["MAXHP"]),
                        (OP_IADD_CLAMP, GUARD, PID["SP"], guard(PID["Level"], GUARD_GT0, k=30), 1, 0, 1000),
                        (OP_ISET, GUARD, PID["SP"], guard(PID["HP"], GUARD_LE0, k=1500), 5, 0, 0)])
        put("Poison", [(OP_IADD_CLAMP, HI_PROP, PID["HP"], 0, -13, 1, PID["MAXHP"]),
                       (OP_IADD_CLAMP, 0, PID["ATK_VALUE"], 0, -900, -5000, 5000),
                       (OP_ISET, GUARD, PID["DEF_VALUE"], guard(PID["ATK_VALUE"], GUARD_LE0, k=-100), 1, 0, 0),
                       (OP_IADD_CLAMP, GUARD, PID["ATK_VALUE"], guard(PID["ATK_VALUE"], GUARD_LE0, k=GUARD_KMIN),
                        9000, -5000, 5000),
                       (OP_ISET, GUARD, PID["DEF_VALUE"], guard(PID["ATK_VALUE"], GUARD_GT0, k=GUARD_KMAX), 777, 0, 0),
                       (OP_ISET, GUARD, PID["Level"], guard(PID["Camp"], GUARD_EQ0, k=2), 61, 0, 0),
                       (OP_IADD_CLAMP, GUARD, PID["SP"], guard(PID["Level"], GUARD_NE0, k=61), -1, 0, 1000)])
    if with_records:
        # skill table: col 1 = cooldown ms (int), col 2 = charge (f64) decays
        lst = [(OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, -100, 0, I64_MAX)]
        if rec_float_op:
            lst.append((OP_RFAFFINE, 0, (0 << 8) | 2, 0, f64bits(0.5), f64bits(0.0), 0))
        if rec_skill_op:  # a third column op (skill id +1, clamped to [1000, 1999]), after cols 1, 2
            lst.append((OP_RIADD_CLAMP, 0, (0 << 8) | 0, 0, 1, 1000, 1999))
        put("SkillCD", lst)
    return ops, n_ops


def _names(lst):
    a = np.zeros((len(lst), 32), np.uint8)
    for i, s in enumerate(lst):
        b = s.encode()
        a[i, :len(b)] = np.frombuffer(b, np.uint8)
    return a


def make_world(n_obj=4096, n_scenes=1, groups_per_scene=16, players_per_group=4, n_ticks=8,
               tick_ms=100, seed=1, ext_frac=0.05, host_ops=True, records=False, rec_rows=64,
               t0=1_700_000_000_000, guid_heads=(7, 9), rec_float_op=True, rec_skill_op=False, sched_edges=False,
               switch_frac=0.0, switch_new_groups=False, rec_steady=False, ext_props=None, burst_frac=0.0,
               burst_props=20, rmw_frac=0.0, spawn_frac=0.0, destroy_frac=0.0, rec_set_frac=0.0,
               rec_set_float=True, obj_props=False, obj_set_frac=0.05, rec_row_frac=0.0, set_ops=False,
               lethal_poison=False, const_guards=False, cell_guards=None):
    """cell_guards=(case, twin[, overrides]): one of the twin worlds of CELL_GUARD_CASES[case] (its world
    options, with the overrides — say a larger n_obj for a timing — replace the ones given here but
    n_ticks and seed): twin "A" guards on mirror int properties, twin "B" on the record cells the
    mirrors track (NFK_GUARD_CELL); see _cell_guard_world."""
    if cell_guards is not None:
        return _cell_guard_world(cell_guards[0], cell_guards[1], n_ticks, seed, *cell_guards[2:])
    if spawn_frac > 0 or destroy_frac > 0:
        return _lifecycle_world(locals())
    rng = np.random.default_rng(seed)
    n_groups = n_scenes * groups_per_scene
    # ---- objects ----
    cell = rng.integers(0, n_groups, n_obj)
    cell[:n_groups] = np.arange(min(n_groups, n_obj))
    scene = (cell // groups_per_scene + 1).astype(np.int32)
    group = (cell % groups_per_scene + 1).astype(np.int32)   # group 0 = scene base group
    ghead = np.where(rng.random(n_obj) < 0.9, guid_heads[0], guid_heads[-1]).astype(np.int64)
    gdata = rng.choice(np.int64(1) << 40, size=n_obj, replace=False).astype(np.int64) + 1
    isplayer = np.zeros(n_obj, np.uint8)
    order = np.lexsort((rng.random(n_obj), cell))
    first = np.ones(n_obj, bool)
    first[1:] = cell[order][1:] != cell[order][:-1]
    idx_in_cell = np.arange(n_obj) - np.maximum.accumulate(np.where(first, np.arange(n_obj), 0))
    isplayer[order[idx_in_cell < players_per_group]] = 1
    cls = np.where(isplayer == 1, CLS_PLAYER, CLS_NPC).astype(np.uint8)

    # ---- creation-time properties ----
    init_i = np.zeros((N_INT, n_obj), np.int64)
    maxhp = rng.integers(500, 5000, n_obj)
    init_i[PID["MAXHP"]] = maxhp
    init_i[PID["HP"]] = rng.integers(1, maxhp + 1)
    if lethal_poison:  # a third of the objects near death
        low = rng.random(n_obj) < 0.33
        init_i[PID["HP"], low] = rng.integers(1, 40, int(low.sum()))
    init_i[PID["HPREGEN"]] = rng.integers(1, 50, n_obj)
    maxmp = rng.integers(100, 1000, n_obj)
    init_i[PID["MAXMP"]] = maxmp
    init_i[PID["MP"]] = rng.integers(0, maxmp + 1)
    init_i[PID["MPREGEN"]] = rng.integers(1, 20, n_obj)
    init_i[PID["MAXSP"]] = rng.integers(100, 300, n_obj)
    init_i[PID["SP"]] = rng.integers(0, 100, n_obj)
    init_i[PID["SPREGEN"]] = rng.integers(1, 5, n_obj)
    init_i[PID["EXP"]] = rng.integers(0, 10 ** 6, n_obj)
    init_i[PID["Gold"]] = rng.integers(0, 10 ** 5, n_obj)
    init_i[PID["Level"]] = rng.integers(1, 60, n_obj)
    init_i[PID["ATK_VALUE"]] = rng.integers(10, 500, n_obj)
    init_i[PID["DEF_VALUE"]] = rng.integers(10, 500, n_obj)
    init_i[PID["Camp"]] = rng.integers(0, 4, n_obj)
    init_i[PID["NPCType"]] = rng.integers(0, 6, n_obj)
    init_i[PID["SceneID"]] = scene   # CreateObject sets SceneID / GroupID (KM:248-249)
    init_i[PID["GroupID"]] = group
    init_f = np.zeros((N_FLT, n_obj), np.float64)

    def coord(n):
        v = rng.uniform(-1000.0, 1000.0, n)
        return np.where(np.abs(v) < 1.0, v + np.sign(v + 0.5) * 2.0, v)  # no near-zero values
    fi = {n: i - N_INT for n, i in PID.items() if i >= N_INT}
    init_f[fi["X"]] = coord(n_obj)
    init_f[fi["Y"]] = coord(n_obj)
    init_f[fi["Z"]] = coord(n_obj)
    init_f[fi["TargetX"]] = coord(n_obj)
    init_f[fi["TargetY"]] = coord(n_obj)
    init_f[fi["AtkDis"]] = rng.uniform(1.0, 10.0, n_obj)
    # a few objects sit exactly on their target: Move produces no change (SetFloat eps path)
    still = rng.random(n_obj) < 0.02
    init_f[fi["X"], still] = init_f[fi["TargetX"], still]

    ops, n_ops = programs(records, rec_float_op, rec_skill_op, set_ops, lethal_poison, const_guards)
    n_kind = len(KINDS) if records else len(KINDS) - 1

    # ---- heartbeats registered before the first frame ----
    spec = [("HPRegen", 1.0, -1), ("MPRegen", 2.0, -1), ("Move", 0.1, -1), ("Patrol", 3.0, -1),
            ("Poison", 0.5, None)]
    s_obj, s_kind, s_int, s_cnt, s_time = [], [], [], [], []
    for name, iv, cnt in spec:
        take = rng.random(n_obj) < (0.7 if name == "Poison" else 1.0)
        objs = np.nonzero(take)[0]
        s_obj.append(objs)
        s_kind.append(np.full(len(objs), KID[name]))
        s_int.append(np.full(len(objs), iv, np.float32))
        s_cnt.append(rng.integers(3, 40, len(objs)) if cnt is None else np.full(len(objs), cnt))
        s_time.append(t0 - rng.integers(0, int(iv * 1000) + 1, len(objs)))
    if records:
        objs = np.nonzero(isplayer)[0]
        s_obj.append(objs)
        s_kind.append(np.full(len(objs), KID["SkillCD"]))
        s_int.append(np.full(len(objs), 0.1, np.float32))
        s_cnt.append(np.full(len(objs), -1))
        s_time.append(t0 - rng.integers(0, 101, len(objs)))
    if sched_edges:
        # reschedule edge cases (SM:71-72): steps that do not fit the hot record's 28-bit field,
        # negative intervals, forever counts whose int32 remain wraps past INT32_MIN within a few
        # frames, and zero counts (never fire)
        for i, (name, iv, cnt) in enumerate(spec):
            m = len(s_obj[i])
            pick = rng.random(m) < 0.05
            if name == "Patrol":      # 2e5 s interval, started long ago: fires, then waits
                s_int[i][pick] = 2.0e5
                s_time[i][pick] = t0 - int(2.0e8) - rng.integers(0, 300, pick.sum())
            elif name == "HPRegen":   # forever, remain wraps INT32_MIN -> INT32_MAX
                s_cnt[i][pick] = -(2 ** 31) + rng.integers(0, 4, pick.sum())
                s_int[i][pick] = 0.05
            elif name == "MPRegen":   # negative interval: next moves backwards, fires every frame
                s_int[i][pick] = -0.05
            elif name == "Poison":    # count 0: registered, never fires
                s_cnt[i][pick] = 0
    s_obj = np.concatenate(s_obj).astype(np.int32)
    perm = rng.permutation(len(s_obj))   # AddSchedule call order is arbitrary
    s_obj = s_obj[perm]
    s_kind = np.concatenate(s_kind).astype(np.int32)[perm]
    s_int = np.concatenate(s_int).astype(np.float32)[perm]
    s_cnt = np.concatenate(s_cnt).astype(np.int32)[perm]
    s_time = np.concatenate(s_time).astype(np.int64)[perm]

    tick_time = (t0 + tick_ms * np.arange(1, n_ticks + 1)).astype(np.int64)

    # ---- SetProperty calls between frames (call order matters) ----
    xt, xo, xp, xb, xm = [], [], [], [], []
    # ext_props: the properties game logic sets ("all": every property but SceneID / GroupID, which
    # only SwitchScene writes, so program operands such as MAXHP / HPREGEN too)
    if ext_props is None:
        ext_props = [PID["HP"], PID["Gold"], PID["EXP"], PID["TargetX"]]
    elif ext_props == "all":
        ext_props = [i for i, n in enumerate(PROPS) if n not in ("SceneID", "GroupID")]
    settable = [i for i, n in enumerate(PROPS) if n not in ("SceneID", "GroupID")]

    def set_values(objs, props):
        """values of SetProperty calls (vectorised): HP within [1, MAXHP], Gold / EXP anything
        up to 1e6, other ints small; 10 % of HP / small-int sets repeat the creation value (no
        change -> no event); floats are coordinates"""
        objs, props = np.asarray(objs, np.int64), np.asarray(props, np.int64)
        n = len(objs)
        hp = rng.integers(1, maxhp[objs] + 1)
        big = rng.integers(0, 10 ** 6, n)
        small = rng.integers(0, 5000, n)
        same = rng.random(n) < 0.1
        fl = coord(n).view(np.int64)
        init = init_i[np.minimum(props, N_INT - 1), objs]
        v = np.where(props == PID["HP"], np.where(same, init, hp),
                     np.where((props == PID["Gold"]) | (props == PID["EXP"]), big,
                              np.where(props < N_INT, np.where(same, init, small), fl)))
        return v.astype(np.int64).view(np.uint64)

    for t in range(n_ticks):
        k = int(ext_frac * n_obj)
        if k > 0:
            objs = rng.integers(0, n_obj, k)
            props = rng.choice(ext_props, k)
            vals = set_values(objs, props)
            # duplicates: same (object, property) set twice in one frame (coalesced)
            dup = rng.random(k) < 0.05
            objs = np.concatenate([objs, objs[dup]])
            props = np.concatenate([props, props[dup]])
            vals = np.concatenate([vals, vals[dup][::-1]])
            xt.append(np.full(len(objs), t))
            xo.append(objs)
            xp.append(props)
            xb.append(vals)
            xm.append(np.zeros(len(objs), np.uint8))
        kb = int(burst_frac * n_obj)
        if kb > 0:
            # bursts: an entity gets `burst_props` distinct properties set in one frame (more than
            # the programs' working set), some of them twice
            bo, bp = [], []
            for o in rng.choice(n_obj, size=min(kb, n_obj), replace=False):
                ps = rng.choice(settable, size=min(burst_props, len(settable)), replace=False)
                ps = np.concatenate([ps, ps[rng.random(len(ps)) < 0.2]])
                bo.append(np.full(len(ps), o))
                bp.append(ps)
            bo, bp = np.concatenate(bo), np.concatenate(bp)
            xt.append(np.full(len(bo), t))
            xo.append(bo)
            xp.append(bp)
            xb.append(set_values(bo, bp))
            xm.append(np.zeros(len(bo), np.uint8))
        kr = int(rmw_frac * n_obj)
        if kr > 0:
            # read-modify-write game logic: SetProperty(p, GetProperty(p) + delta) (x_mode 1: x_bits is
            # the delta), half of them twice on the same (entity, property) in the same window, so
            # the second Get must see the first Set (KM:401 after KM:323)
            ro = rng.integers(0, n_obj, kr)
            rp = rng.choice(ext_props, kr)
            again = rng.random(kr) < 0.5
            ro = np.concatenate([ro, ro[again]])
            rp = np.concatenate([rp, rp[again]])
            di = rng.integers(-50, 51, len(ro))
            di[di == 0] = 7
            df = rng.uniform(-5.0, 5.0, len(ro)).view(np.int64)
            xt.append(np.full(len(ro), t))
            xo.append(ro)
            xp.append(rp)
            xb.append(np.where(rp < N_INT, di, df).astype(np.int64).view(np.uint64))
            xm.append(np.ones(len(ro), np.uint8))
    cat = lambda lst, dt: np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
    x_tick, x_obj, x_pid, x_bits = cat(xt, np.int32), cat(xo, np.int32), cat(xp, np.int32), cat(xb, np.uint64)
    x_mode = cat(xm, np.uint8)
    obj_extra = {}
    if obj_props:
        obj_extra, (x_tick, x_obj, x_pid, x_bits, x_mode) = _object_props(
            rng, n_obj, n_ticks, ghead, gdata, obj_set_frac, x_tick, x_obj, x_pid, x_bits, x_mode)

    # ---- AddSchedule / RemoveSchedule calls between frames ----
    ht, hop, hob, hk, hiv, hc, htm = [], [], [], [], [], [], []
    if host_ops:
        for t in range(1, n_ticks):
            m = max(1, n_obj // 64)
            o = rng.integers(0, n_obj, m)
            r = rng.random(m)
            rm_kind = rng.choice([KID["Patrol"], KID["Poison"], KID["MPRegen"]], m)
            add_kind = rng.choice([KID["HPRegen"], KID["Patrol"]], m)
            op = np.where(r < 0.45, 1, np.where(r < 0.75, 2, np.where(r < 0.85, 3, 1)))
            kind = np.where(r < 0.45, KID["Poison"], np.where(r < 0.75, rm_kind, np.where(r < 0.85, 0, add_kind)))
            ht.append(np.full(m, t))
            hop.append(op)
            hob.append(o)
            hk.append(kind)
            hiv.append(np.where(kind == KID["Poison"], 0.5, 1.0))
            hc.append(np.where(kind == KID["Poison"], rng.integers(1, 5, m), -1))
            htm.append(int(tick_time[t - 1]) + rng.integers(0, tick_ms, m))
    cat1 = lambda lst: np.concatenate(lst) if lst else np.zeros(0)
    ht, hop, hob, hk, hiv, hc, htm = (cat1(x) for x in (ht, hop, hob, hk, hiv, hc, htm))
    h = dict(h_tick=np.array(ht, np.int32), h_op=np.array(hop, np.int32), h_obj=np.array(hob, np.int32),
             h_kind=np.array(hk, np.int32), h_interval=np.array(hiv, np.float32),
             h_count=np.array(hc, np.int32), h_time=np.array(htm, np.int64))

    # ---- SwitchScene calls between frames (KM:901): at most one per object per frame, made
    #      before the frame's other calls; targets are other cells of any scene, sometimes the
    #      object's own cell, and (switch_new_groups) groups that do not exist yet ----
    st, so, ss, sg, sx, sy, sz = [], [], [], [], [], [], []
    if switch_frac > 0:
        for t in range(1, n_ticks):
            k = max(1, int(switch_frac * n_obj))
            objs = rng.choice(n_obj, size=min(k, n_obj), replace=False)
            for o in objs:
                r = rng.random()
                if r < 0.1:
                    tc, tg = None, None          # own cell: property writes only
                elif switch_new_groups and r < 0.2:
                    tc = int(rng.integers(0, n_groups))
                    tg = groups_per_scene + 1 + int(rng.integers(0, 3))
                else:
                    tc, tg = int(rng.integers(0, n_groups)), None
                st.append(t)
                so.append(o)
                ss.append(-1 if tc is None else tc // groups_per_scene + 1)
                sg.append(-1 if tc is None else (tg if tg is not None else tc % groups_per_scene + 1))
                sx.append(np.float32(rng.uniform(-500, 500)))
                sy.append(np.float32(rng.uniform(-500, 500)))
                sz.append(np.float32(rng.uniform(0, 50)))
    sw = dict(sw_tick=np.array(st, np.int32), sw_obj=np.array(so, np.int32), sw_scene=np.array(ss, np.int32),
              sw_group=np.array(sg, np.int32), sw_x=np.array(sx, np.float32), sw_y=np.array(sy, np.float32),
              sw_z=np.array(sz, np.float32))

    n_rec = 1 if records else 0
    extra = {"x_mode": x_mode} if rmw_frac > 0 else {}
    n_op = len(OBJ_PROPS) if obj_props else 0
    w = dict(**extra, **obj_extra,
        cfg=np.array([n_obj, N_INT, N_FLT, 2, n_kind, n_rec, len(s_obj), n_ticks], np.int64),
        prop_flags=_prop_flags(n_op), prop_names=_names(PROPS + OBJ_PROPS[:n_op]), kind_names=_names(KINDS[:n_kind]),
        ops=ops[:n_kind].copy(), n_ops=n_ops[:n_kind].copy(),
        guid_head=ghead, guid_data=gdata, scene=scene, group=group, cls=cls, is_player=isplayer,
        init_i=init_i, init_f=init_f,
        s_obj=s_obj, s_kind=s_kind, s_interval=s_int, s_count=s_cnt, s_time=s_time,
        tick_time=tick_time, x_tick=x_tick, x_obj=x_obj, x_pid=x_pid, x_bits=x_bits, **h, **sw,
        scene_props=np.array([PID["SceneID"], PID["GroupID"], PID["X"], PID["Y"], PID["Z"]], np.int32))
    if records:
        rows, cols = rec_rows, 3
        w["rec_rows"] = np.array([rows], np.int32)
        w["rec_cols"] = np.array([cols], np.int32)
        ct = np.zeros((1, MAX_REC_COLS), np.uint8)
        ct[0, 2] = 1                                   # col 0 skill id, 1 cooldown ms, 2 charge (f64)
        w["rec_ctype"] = ct
        rf = np.zeros((2, 1), np.uint8)
        rf[CLS_PLAYER, 0] = PRIVATE                    # skill table: private to its owner
        rf[CLS_NPC, 0] = PUBLIC | PRIVATE
        w["rec_flags"] = rf
        cells = np.zeros((n_obj, cols, rows), np.uint64)
        cells[:, 0, :] = rng.integers(1000, 2000, (n_obj, rows)).astype(np.uint64)
        # rec_steady: cooldowns of hours and charges far above the threshold, so that every frame
        # of a bench run updates the same share of cells (the default decays within ~30 frames)
        cd = rng.integers(0, 3000, (n_obj, rows)) + (3_600_000 if rec_steady else 0)
        cd[rng.random((n_obj, rows)) < 0.3] = 0
        cells[:, 1, :] = cd.astype(np.uint64)
        ch = rng.uniform(0.0, 100.0, (n_obj, rows)) * (2.0 ** 200 if rec_steady else 1.0)
        ch[rng.random((n_obj, rows)) < 0.2] = 0.0005    # below the 0.001 record threshold
        cells[:, 2, :] = ch.view(np.uint64)
        used = rng.integers(0, 2 ** 63, n_obj, dtype=np.int64).astype(np.uint64)
        if rows < 64:
            used &= np.uint64((1 << rows) - 1)
        w["rec0_cells"] = cells
        w["rec0_used"] = used
        if rec_set_frac > 0 or rec_row_frac > 0:
            w.update(_record_sets(rng, n_obj, n_ticks, rows, cols, rec_set_frac, rec_set_float, rec_row_frac))
    return w


def _object_props(rng, n_obj, n_ticks, ghead, gdata, frac, x_tick, x_obj, x_pid, x_bits, x_mode):
    """Object (NFGUID) properties: creation-time values (init_oh / init_od: other objects of the
    world, or the null NFGUID) and NFIKernelModule::SetPropertyObject calls (KM:362) merged into the
    SetProperty call stream of each window (x_pid >= N_INT + N_FLT, x_bits = nData64, x_bits_h =
    nHead64; 0 for the int / f64 calls).  Values: another object's GUID, the null GUID, the current
    value again (no change, PR:396), or a GUID that differs from the current one in its head half only
    (NFGUID::operator== compares both halves)."""
    no = len(OBJ_PROPS)
    base = N_INT + N_FLT
    pick = rng.integers(0, n_obj, (no, n_obj))
    null = rng.random((no, n_obj)) < 0.3
    init_oh = np.where(null, 0, ghead[pick]).astype(np.int64)
    init_od = np.where(null, 0, gdata[pick]).astype(np.int64)
    x_bits_h = np.zeros(len(x_tick), np.uint64)
    cur_h, cur_d = init_oh.copy(), init_od.copy()   # (the generator's view: only these calls change them)
    ts, os_, ps, bs, hs = [], [], [], [], []
    for t in range(n_ticks):
        k = int(frac * n_obj)
        if k <= 0:
            continue
        o = rng.integers(0, n_obj, k)
        p = rng.integers(0, no, k)
        again = rng.random(k) < 0.1                      # the same (object, property) twice
        o, p = np.concatenate([o, o[again]]), np.concatenate([p, p[again]])
        r = rng.random(len(o))
        q = rng.integers(0, n_obj, len(o))
        vh = ghead[q].astype(np.int64)
        vd = gdata[q].astype(np.int64)
        vh = np.where(r < 0.15, 0, vh)                   # the null NFGUID
        vd = np.where(r < 0.15, 0, vd)
        same = (r >= 0.15) & (r < 0.3)                   # the value it holds: no change, no event
        vh = np.where(same, cur_h[p, o], vh)
        vd = np.where(same, cur_d[p, o], vd)
        headonly = (r >= 0.3) & (r < 0.4)                # head half differs only
        vh = np.where(headonly, cur_h[p, o] ^ 3, vh)
        vd = np.where(headonly, cur_d[p, o], vd)
        for i in range(len(o)):
            cur_h[p[i], o[i]], cur_d[p[i], o[i]] = vh[i], vd[i]
        ts.append(np.full(len(o), t))
        os_.append(o)
        ps.append(base + p)
        bs.append(vd.view(np.uint64))
        hs.append(vh.view(np.uint64))
    if ts:
        ot, oo, op_, ob, oh = (np.concatenate(x) for x in (ts, os_, ps, bs, hs))
        # interleave with the window's other Set calls: order by tick, random within a tick
        t_all = np.concatenate([x_tick, ot]).astype(np.int32)
        key = np.lexsort((rng.random(len(t_all)), t_all))
        x_tick = t_all[key]
        x_obj = np.concatenate([x_obj, oo]).astype(np.int32)[key]
        x_pid = np.concatenate([x_pid, op_]).astype(np.int32)[key]
        x_bits = np.concatenate([x_bits, ob]).astype(np.uint64)[key]
        x_mode = np.concatenate([x_mode, np.zeros(len(ot), np.uint8)])[key]
        x_bits_h = np.concatenate([x_bits_h, oh]).astype(np.uint64)[key]
    extra = dict(n_oprops=np.array([no], np.int64), init_oh=init_oh, init_od=init_od, x_bits_h=x_bits_h)
    return extra, (x_tick, x_obj, x_pid, x_bits, x_mode)


def _record_sets(rng, n_obj, n_ticks, rows, cols, frac, with_float, row_frac=0.0):
    """NFIKernelModule::SetRecordInt / SetRecordFloat calls between frames (r_*, call order within
    a window): random (object, row, col) cells of record 0 — rows used or not (a Set on an unused
    row is refused, RC:194) — with a third of them set twice in the window (coalesced to one event)
    and some set to the value they already hold (no event).  with_float=False keeps to the int
    columns (the reference's own NFCRecord::SetFloat is broken, see test_reference_record_setfloat_bug)."""
    rt, ro, rr, rw, rc, rb, rop, rv = [], [], [], [], [], [], [], []
    ncol = cols if with_float else 2
    for t in range(1, n_ticks):
        k = int(frac * n_obj)
        kr = int(row_frac * n_obj)
        if k <= 0 and kr <= 0:
            continue
        o = rng.integers(0, n_obj, k)
        row = rng.integers(0, rows, k)
        col = rng.integers(0, ncol, k)
        again = rng.random(k) < 0.33
        o, row, col = (np.concatenate([x, x[again]]) for x in (o, row, col))
        iv = rng.integers(0, 5000, len(o)).astype(np.int64)
        iv[rng.random(len(o)) < 0.1] = 0                 # often the value a cooldown already holds
        fv = rng.uniform(-50.0, 50.0, len(o))
        bits = np.where(col == 2, fv.view(np.int64), iv).astype(np.int64).view(np.uint64)
        op = np.zeros(len(o), np.uint8)
        vals = np.zeros((len(o), MAX_REC_COLS), np.uint64)
        if kr > 0:
            # record row operations (NFCRecord::AddRow / Remove, NFCKernelModule::ClearRecord): AddRow
            # at the first unused row (-1) or at a given row (a used one is covered), Remove of used
            # and unused rows, Clear; their objects also get SetRecord calls in the same window
            qo = np.concatenate([rng.integers(0, n_obj, kr // 2), o[:kr - kr // 2]]) if k else rng.integers(0, n_obj, kr)
            r = rng.random(len(qo))
            qop = np.where(r < 0.45, 1, np.where(r < 0.88, 2, 3)).astype(np.uint8)
            qrow = rng.integers(0, rows, len(qo))
            qrow[(qop == 1) & (rng.random(len(qo)) < 0.5)] = -1
            qv = np.zeros((len(qo), MAX_REC_COLS), np.uint64)
            qv[:, 0] = rng.integers(1000, 2000, len(qo)).astype(np.uint64)
            qv[:, 1] = rng.integers(0, 3000, len(qo)).astype(np.uint64)
            qv[:, 2] = rng.uniform(0.0, 100.0, len(qo)).view(np.uint64)
            o = np.concatenate([o, qo])
            row = np.concatenate([row, qrow])
            col = np.concatenate([col, np.zeros(len(qo), np.int64)])
            bits = np.concatenate([bits, np.zeros(len(qo), np.uint64)])
            op = np.concatenate([op, qop])
            vals = np.concatenate([vals, qv])
        perm = rng.permutation(len(o))                   # call order within the window
        rt.append(np.full(len(o), t))
        ro.append(o[perm])
        rr.append(row[perm])
        rw.append(col[perm])
        rb.append(bits[perm])
        rop.append(op[perm])
        rv.append(vals[perm])
    cat = lambda lst, dt: np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
    n = sum(len(x) for x in rt)
    out = dict(r_tick=cat(rt, np.int32), r_obj=cat(ro, np.int32), r_rec=np.zeros(n, np.int32),
               r_row=cat(rr, np.int32), r_col=cat(rw, np.int32), r_bits=cat(rb, np.uint64))
    if row_frac > 0:
        out["r_op"] = cat(rop, np.uint8)
        out["r_vals"] = np.concatenate(rv).astype(np.uint64) if rv else np.zeros((0, MAX_REC_COLS), np.uint64)
    return out


def _lifecycle_world(kw):
    """make_world with objects created and destroyed between frames (NFCKernelModule::CreateObject
    after start, KM:101-271; DestroyObject, KM:273-308).  Every frame t >= 1, spawn_frac x n_obj new
    objects are created (appended to the object arrays in call order, `born` = t; they get their
    AddSchedule calls in the same window, after the creation) and destroy_frac x n_obj live objects
    are destroyed (`d_tick`, `d_obj`, the window's last calls).  A window's calls run: creations,
    SwitchScene, schedule calls, SetProperty calls, destructions.  Calls on an object before its
    creation or after its destruction are dropped, and so are schedule and SwitchScene calls in its
    destruction window (the reference would keep an AddSchedule queued for an object destroyed in
    the same window as a schedule of a dead GUID)."""
    kw = dict(kw)
    spawn_frac, destroy_frac = kw.pop("spawn_frac"), kw.pop("destroy_frac")
    n0, n_ticks, seed = kw["n_obj"], kw["n_ticks"], kw["seed"]
    per = int(spawn_frac * n0)
    n_new = per * max(n_ticks - 1, 0)
    kw["n_obj"] = n0 + n_new
    w = make_world(**kw, spawn_frac=0.0, destroy_frac=0.0)
    rng = np.random.default_rng(seed + 991)
    N = n0 + n_new
    born = np.full(N, -1, np.int32)
    for t in range(1, n_ticks):
        born[n0 + (t - 1) * per: n0 + t * per] = t
    # destructions: live objects (born before the window), each destroyed once
    died = np.full(N, 1 << 30, np.int64)
    dt, do = [], []
    kd = int(destroy_frac * n0)
    for t in range(1, n_ticks):
        cand = np.nonzero((born < t) & (died > t))[0]
        pick = rng.choice(cand, size=min(kd, len(cand)), replace=False) if kd and len(cand) else np.zeros(0, np.int64)
        died[pick] = t
        dt.append(np.full(len(pick), t))
        do.append(np.sort(pick))
    d_tick = np.concatenate(dt).astype(np.int32) if dt else np.zeros(0, np.int32)
    d_obj = np.concatenate(do).astype(np.int32) if do else np.zeros(0, np.int32)

    def alive_at(o, t, last_window_ok):
        b = born[o]
        ok = (b < 0) | (b <= t)
        return ok & ((t < died[o]) | (last_window_ok & (t == died[o])))

    # calls: SetProperty allowed in the destruction window (dropped with the object), schedule and
    # SwitchScene calls not
    keep = alive_at(w["x_obj"], w["x_tick"], True)
    for k in ("x_tick", "x_obj", "x_pid", "x_bits", "x_mode", "x_bits_h"):
        if k in w:
            w[k] = w[k][keep]
    if "r_tick" in w:   # SetRecord* calls: like SetProperty
        keep = alive_at(w["r_obj"], w["r_tick"], True)
        for k in ("r_tick", "r_obj", "r_rec", "r_row", "r_col", "r_bits", "r_op", "r_vals"):
            if k in w:
                w[k] = w[k][keep]
    keep = alive_at(w["h_obj"], w["h_tick"], False)
    for k in ("h_tick", "h_op", "h_obj", "h_kind", "h_interval", "h_count", "h_time"):
        w[k] = w[k][keep]
    keep = alive_at(w["sw_obj"], w["sw_tick"], False)
    for k in ("sw_tick", "sw_obj", "sw_scene", "sw_group", "sw_x", "sw_y", "sw_z"):
        w[k] = w[k][keep]
    # the late objects' AddSchedule calls move from before frame 0 to their creation window
    late = born[w["s_obj"]] >= 0
    s_late = {k: w[k][late] for k in ("s_obj", "s_kind", "s_interval", "s_count", "s_time")}
    for k in ("s_obj", "s_kind", "s_interval", "s_count", "s_time"):
        w[k] = w[k][~late]
    bt = born[s_late["s_obj"]]
    order = np.argsort(bt, kind="stable")
    tt = w["tick_time"]
    st_late = s_late["s_time"][order]
    st_min = st_late.min() if len(st_late) else 0   # (a destroy-only world has no late objects)
    h_new = dict(h_tick=bt[order], h_op=np.ones(len(order), np.int32), h_obj=s_late["s_obj"][order],
                 h_kind=s_late["s_kind"][order], h_interval=s_late["s_interval"][order],
                 h_count=s_late["s_count"][order],
                 h_time=(tt[np.maximum(bt[order] - 1, 0)] + (st_late - st_min) % 100).astype(np.int64))
    # the window's schedule calls: the creations' AddSchedule first, then the generator's
    ht = np.concatenate([h_new["h_tick"], w["h_tick"]])
    first = np.concatenate([np.zeros(len(order), np.int8), np.ones(len(w["h_tick"]), np.int8)])
    o2 = np.lexsort((first, ht))
    for k in h_new:
        w[k] = np.concatenate([h_new[k], w[k]])[o2].astype(w[k].dtype)
    w["cfg"][6] = len(w["s_obj"])
    if int(w["cfg"][5]):   # late objects start with empty records
        w["rec0_cells"][born >= 0] = 0
        w["rec0_used"][born >= 0] = 0
    w["born"] = born
    w["d_tick"], w["d_obj"] = d_tick, d_obj
    return w


# ---- twin worlds for guards on record cells (NFK_GUARD_CELL) ---------------------------------
# Twin A guards on MIRROR int properties, twin B — the same workload byte for byte but for the guard
# words — on the record cells the mirrors track.  Each mirror equals its cell's NFCRecord::GetInt value
# (the cell, or 0 where the record does not use the row, RC:616-635) at every point a guard can read it:
# it starts equal; a RIADD_CLAMP on the guard's column sits next to an IADD_CLAMP of the same delta and
# bounds on each mirror of that column, in the same program; every window whose record calls change a
# guard cell's GetInt value carries a SetPropertyInt of the mirror to the value the calls leave
# (SetRecordInt -> its value, Remove / ClearRecord -> 0, AddRow -> the row's value); the random
# SetProperty calls skip the mirrors.  Where an op would move 0 (a clamp with lo > 0) the mirror has no
# op and the cells hold the op's fixed point, with no row calls.  Both twins carry the mirrored ops and
# calls, so their outputs are identical in full.
def _cg_programs(case):
    """(guard cells [(rec, row, col)], mirrors [property], programs {kind: [op]}) of a case; an op's
    guard is 0 or ("G", cell index, comparison, {k= | vs=})"""
    P = PID
    g = lambda c, cmp, **kw: ("G", c, cmp, kw)
    hp_up = (OP_IADD_CLAMP, 0, P["HP"], 0, 5, 0, 5000)
    hp_dn = (OP_IADD_CLAMP, 0, P["HP"], 0, -13, 1, 5000)
    lerp = (OP_FLERP, 0, P["X"], 0, P["TargetX"], f64bits(0.125), 0)
    cd = (OP_RIADD_CLAMP, 0, (0 << 8) | 1, 0, -100, 0, I64_MAX)
    charge = (OP_RFAFFINE, 0, (0 << 8) | 2, 0, f64bits(0.5), f64bits(0.0), 0)
    mcd = lambda m: (OP_IADD_CLAMP, 0, P[m], 0, -100, 0, I64_MAX)   # the mirror's twin of `cd`
    if case in ("static", "calls"):
        rows = 20 if case == "static" else 32
        cells = [(0, 0, 1), (0, rows // 2 - 1, 1), (0, rows - 1, 1)]
        mirrors = ["MAXSP", "SPREGEN", "NPCType"]
        progs = {
            "HPRegen": [hp_up,
                        (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_GT0, k=30), 1, 0, 1 << 40),
                        (OP_ISET, GUARD, P["EXP"], g(1, GUARD_LE0, k=-100), 5, 0, 0)],
            "MPRegen": [(OP_ISET, GUARD, P["EXP"], g(2, GUARD_NE0), 7, 0, 0),
                        (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_EQ0), 3, 0, 1 << 40)],
            "Move": [lerp, (OP_FSET, A_PROP | GUARD, P["Z"], g(1, GUARD_GT0, k=30), P["TargetX"], 0, 0)],
            "Patrol": [(OP_IADD_CLAMP, GUARD, P["Gold"], g(2, GUARD_GT0, vs=P["Level"]), -2, 0, 1 << 40)],
            "Poison": [hp_dn,
                       (OP_ISET, GUARD, P["EXP"], g(0, GUARD_GT0, k=GUARD_KMIN), 9, 0, 0),
                       (OP_IADD_CLAMP, GUARD, P["EXP"], g(1, GUARD_LE0, k=GUARD_KMAX), 3, 0, 1 << 40),
                       (OP_ISET, GUARD, P["Gold"], g(2, GUARD_LE0, k=-100), 1, 0, 0),
                       (OP_IADD_CLAMP, GUARD, P["Gold"], g(2, GUARD_EQ0, k=30), 11, 0, 1 << 40)],
            "SkillCD": [cd, charge] + [mcd(m) for m in mirrors]}
    elif case == "replay":
        # the record op in Move (every object, every frame): before a guarded op of its own program and
        # before the guarded kinds Patrol and Poison; HPRegen, before both, sees the frame-start cell
        cells, mirrors = [(0, 63, 1)], ["MAXSP"]
        progs = {
            "HPRegen": [hp_up, (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_LE0, k=1500), 1, 0, 1 << 40)],
            "MPRegen": [(OP_IADD_CLAMP, 0, P["MP"], 0, 1, 0, 1000)],
            "Move": [lerp, cd, mcd("MAXSP"),
                     (OP_ISET, GUARD, P["EXP"], g(0, GUARD_LE0, k=1500), 1, 0, 0),
                     (OP_ISET, GUARD, P["EXP"], g(0, GUARD_GT0, k=1500), 2, 0, 0)],
            "Patrol": [(OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_NE0), 7, 0, 1 << 40)],
            "Poison": [hp_dn, (OP_IADD_CLAMP, GUARD, P["EXP"], g(0, GUARD_GT0, k=700), 3, 0, 1 << 40)],
            "SkillCD": [charge]}
    elif case == "unused_row_fixed_point":
        # RIADD_CLAMP +1 [1000, 1999] on cells that all hold 1999: the op changes nothing, and would
        # lift an unused row's 0 to 1000 if the replay touched it; the mirror has no op
        cells, mirrors = [(0, 5, 0)], ["MAXSP"]
        progs = {
            "HPRegen": [hp_up, (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_EQ0), 1, 0, 1 << 40)],
            "MPRegen": [(OP_IADD_CLAMP, 0, P["MP"], 0, 1, 0, 1000)],
            "Move": [lerp, (OP_RIADD_CLAMP, 0, (0 << 8) | 0, 0, 1, 1000, 1999),
                     (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_EQ0), 1, 0, 1 << 40),
                     (OP_IADD_CLAMP, GUARD, P["EXP"], g(0, GUARD_GT0), 1, 0, 1 << 40)],
            "Patrol": [(OP_ISET, GUARD, P["EXP"], g(0, GUARD_EQ0), 0, 0, 0)],
            "Poison": [hp_dn, (OP_IADD_CLAMP, GUARD, P["Gold"], g(0, GUARD_GT0), -3, 0, 1 << 40)],
            "SkillCD": [cd, charge]}
    else:
        raise ValueError(f"unknown cell-guard case {case!r}")
    return cells, mirrors, progs


CELL_GUARD_CASES = {
    # 4097 objects in 5 x 13 groups: a ragged last tile, tiles straddling segments, slack slots
    "static": dict(n_obj=4097, n_scenes=5, groups_per_scene=13, rec_rows=20),
    "replay": dict(n_obj=3000, n_scenes=2, groups_per_scene=8, rec_rows=64),
    "unused_row_fixed_point": dict(n_obj=3000, n_scenes=2, groups_per_scene=8, rec_rows=16, fixed_col0=1999),
    # SetRecordInt on the guard cells in every window, Remove / AddRow / ClearRecord on the guard rows,
    # with spawn, destroy and SwitchScene
    "calls": dict(n_obj=3000, n_scenes=2, groups_per_scene=8, rec_rows=32, spawn_frac=0.02, destroy_frac=0.02,
                  switch_frac=0.02, rec_set_frac=0.05, rec_set_float=False, rec_row_frac=0.03, cell_calls=0.15),
}


def _cell_guard_world(case, twin, n_ticks, seed, overrides=None):
    assert twin in ("A", "B")
    opt = dict(CELL_GUARD_CASES[case], **(overrides or {}))
    fixed_col0, cell_calls = opt.pop("fixed_col0", None), opt.pop("cell_calls", 0.0)
    w = make_world(n_ticks=n_ticks, seed=seed, records=True, ext_props="all", ext_frac=0.05, **opt)
    cells, mirrors, progs = _cg_programs(case)
    mpid = [PID[m] for m in mirrors]
    rows = int(w["rec_rows"][0])
    N = len(w["guid_head"])
    rng = np.random.default_rng(seed + 4242)
    if fixed_col0 is not None:
        w["rec0_cells"][:, 0, :] = np.uint64(fixed_col0)
    # the guard rows are used on about half the objects (make_world's masks never use row 63; objects
    # created after the start keep their empty records)
    for row in sorted({c[1] for c in cells}):
        on = (rng.random(N) < 0.5) & ((w["born"] < 0) if "born" in w else True)
        bit = np.uint64(1) << np.uint64(row)
        w["rec0_used"] = np.where(on, w["rec0_used"] | bit, w["rec0_used"] & ~bit).astype(np.uint64)
    # ---- programs: the guards on the mirrors (A) or on the cells (B) ----
    ops = np.zeros((len(KINDS), MAX_OPS), OP_DTYPE)
    n_ops = np.zeros(len(KINDS), np.int32)
    for kind, lst in progs.items():
        for i, (code, flags, dst, gd, a, b, c) in enumerate(lst):
            if gd:
                _, ci, cmp, kw = gd
                if twin == "A":
                    gd = guard(mpid[ci], cmp, **kw)
                else:
                    gd, flags = guard_cell(*cells[ci], cmp, **kw), flags | GUARD_CELL
            ops[KID[kind], i] = (code, flags, dst, gd, a, b, c)
        n_ops[KID[kind]] = len(lst)
    w["ops"], w["n_ops"] = ops, n_ops
    # ---- the random SetProperty calls skip the mirrors ----
    keep = ~np.isin(w["x_pid"], mpid)
    for k in ("x_tick", "x_obj", "x_pid", "x_bits"):
        w[k] = w[k][keep]
    born = w["born"] if "born" in w else np.full(N, -1, np.int32)
    died = np.full(N, 1 << 30, np.int64)
    if "d_tick" in w:
        died[w["d_obj"]] = w["d_tick"]
    # ---- SetRecordInt calls on the guard cells, every window: rows used or not, values the cell
    #      already holds (the same value again in the next window, and twice in one window) ----
    if cell_calls > 0:
        rt, ro, rr, rc, rb = [], [], [], [], []
        prev = None
        for t in range(1, n_ticks):
            alive = np.nonzero(((born < 0) | (born <= t)) & (t <= died))[0]
            o = rng.choice(alive, size=max(1, int(cell_calls * len(alive))))
            ci = rng.integers(0, len(cells), len(o))
            v = np.where(rng.random(len(o)) < 0.3, 0, rng.integers(0, 3000, len(o))).astype(np.uint64)
            if prev is not None:   # what the last window set, again (the objects still alive)
                po, pc, pv = prev
                ok = t <= died[po]
                o, ci, v = np.concatenate([o, po[ok]]), np.concatenate([ci, pc[ok]]), np.concatenate([v, pv[ok]])
            twice = rng.random(len(o)) < 0.2
            o, ci, v = (np.concatenate([x, x[twice]]) for x in (o, ci, v))
            prev = (o[:len(o) // 3], ci[:len(o) // 3], v[:len(o) // 3])
            cr = np.array([c[1] for c in cells])[ci]
            cc = np.array([c[2] for c in cells])[ci]
            rt.append(np.full(len(o), t)), ro.append(o), rr.append(cr), rc.append(cc), rb.append(v)
        cat = lambda a, b, dt: np.concatenate([a] + b).astype(dt)
        n_add = sum(len(x) for x in rt)
        tick = cat(w["r_tick"], rt, np.int32)
        order = np.argsort(tick, kind="stable")   # behind the window's other record calls
        w["r_tick"] = tick[order]
        w["r_obj"] = cat(w["r_obj"], ro, np.int32)[order]
        w["r_rec"] = cat(w["r_rec"], [np.zeros(n_add)], np.int32)[order]
        w["r_row"] = cat(w["r_row"], rr, np.int32)[order]
        w["r_col"] = cat(w["r_col"], rc, np.int32)[order]
        w["r_bits"] = cat(w["r_bits"], rb, np.uint64)[order]
        if "r_op" in w:
            w["r_op"] = cat(w["r_op"], [np.zeros(n_add)], np.uint8)[order]
            w["r_vals"] = np.concatenate([w["r_vals"], np.zeros((n_add, MAX_REC_COLS), np.uint64)])[order]
    # ---- the mirrors: creation values, then one SetPropertyInt per window and mirror whose cell's
    #      GetInt value the window's record calls changed (the used masks replayed call by call) ----
    used = w["rec0_used"].astype(np.uint64).copy()
    for ci, (_, row, col) in enumerate(cells):
        on = ((used >> np.uint64(row)) & np.uint64(1)).astype(bool)
        w["init_i"][mpid[ci]] = np.where(on, w["rec0_cells"][:, col, row].view(np.int64), 0)
    if "r_tick" in w:
        um = [int(x) for x in used]
        rowm = (1 << rows) - 1
        by_row = {}
        for ci, (_, row, col) in enumerate(cells):
            by_row.setdefault(row, []).append((ci, col))
        r_op = w["r_op"] if "r_op" in w else np.zeros(len(w["r_tick"]), np.uint8)
        xt, xo, xp, xb = [], [], [], []
        for t in range(1, n_ticks):
            final = {}   # (object, cell) -> the GetInt value the window's calls leave

            def unuse(o, row):
                if (um[o] >> row) & 1:
                    um[o] &= ~(1 << row)
                    for ci, _ in by_row.get(row, ()):
                        final[(o, ci)] = 0
            for i in np.nonzero(w["r_tick"] == t)[0]:
                o, row, col, op = int(w["r_obj"][i]), int(w["r_row"][i]), int(w["r_col"][i]), int(r_op[i])
                if op == 0:      # SetRecordInt: refused on an unused row (RC:194)
                    if (um[o] >> row) & 1:
                        for ci, c in by_row.get(row, ()):
                            if c == col:
                                final[(o, ci)] = int(w["r_bits"][i])
                elif op == 1:    # AddRow: the first unused row (-1), or the given one (covered)
                    if row < 0:
                        free = ~um[o] & rowm
                        if not free:
                            continue
                        row = (free & -free).bit_length() - 1
                    um[o] |= 1 << row
                    for ci, c in by_row.get(row, ()):
                        final[(o, ci)] = int(w["r_vals"][i, c])
                elif op == 2:
                    unuse(o, row)
                else:            # ClearRecord
                    for r in range(rows):
                        unuse(o, r)
            for (o, ci), v in sorted(final.items()):
                xt.append(t), xo.append(o), xp.append(mpid[ci]), xb.append(v)
        tick = np.concatenate([w["x_tick"], np.array(xt, np.int32)]).astype(np.int32)
        order = np.argsort(tick, kind="stable")
        w["x_tick"] = tick[order]
        w["x_obj"] = np.concatenate([w["x_obj"], np.array(xo, np.int32)]).astype(np.int32)[order]
        w["x_pid"] = np.concatenate([w["x_pid"], np.array(xp, np.int32)]).astype(np.int32)[order]
        w["x_bits"] = np.concatenate([w["x_bits"], np.array(xb, np.uint64)]).astype(np.uint64)[order]
    w["cg_cells"] = np.array(cells, np.int32)
    w["cg_mirrors"] = np.array(mpid, np.int32)
    return w


def bench_world(n_obj=1 << 20, groups=4096, players_per_group=8, n_ticks=16, seed=2026, **kw):
    """config[1]: 1M NPCs in one scene, 4096 groups, int/float mutation + diff + fan-out."""
    return make_world(n_obj=n_obj, n_scenes=1, groups_per_scene=groups,
                      players_per_group=players_per_group, n_ticks=n_ticks, seed=seed,
                      ext_frac=kw.pop("ext_frac", 0.0), host_ops=kw.pop("host_ops", False), **kw)


def fanout_world(n_ticks=4, seed=2027, n_obj=1 << 21, scenes=256, groups=64, players_per_group=32, **kw):
    """config[3]: 256 scenes x 64 groups, 2M entities; 32 players per group, so every public dirty
    property fans out to 31 recipients (scene-group sync-list dominated)."""
    return make_world(n_obj=n_obj, n_scenes=scenes, groups_per_scene=groups, players_per_group=players_per_group,
                      n_ticks=n_ticks, seed=seed, ext_frac=kw.pop("ext_frac", 0.0),
                      host_ops=kw.pop("host_ops", False), **kw)


def record_world(n_ticks=4, seed=2028, n_obj=500_000, groups=31_250, rec_rows=64, steady=False, **kw):
    """config[4]: 500k players, each with a 64-row skill record whose cooldown (int) and charge
    (f64) columns a 100 ms SkillCD heartbeat updates every frame; groups of 16 players."""
    per = n_obj // groups
    return make_world(n_obj=n_obj, n_scenes=1, groups_per_scene=groups, players_per_group=per, n_ticks=n_ticks,
                      seed=seed, records=True, rec_rows=rec_rows, ext_frac=kw.pop("ext_frac", 0.0),
                      host_ops=kw.pop("host_ops", False), rec_steady=steady, **kw)


# ---- BASELINE config[0]: Tutorial3 scaled to 10k NPCs ----------------------------------------
# Tutorial/Tutorial3/HelloWorld3Module.cpp: on COE_CREATE_HASDATA every object gets the heartbeat
# AddSchedule(self, "OnHeartBeat", 5.0f, 10) (:49-56) and an int property "World" with a property
# callback (:96-104, OnPropertyCallBackEvent); game events set "World" (:16-22, OnEvent).  Scaled
# to 10k NPC objects in scene 1 group 0.  The tutorial's heartbeat only prints (:24-34), so its
# device program is empty: the frame scans the schedules, reschedules the fired ones and hands them
# to the host functor (the fired list), and the OnEvent Sets of "World" are the dirty events.
# (world_effect=True gives the heartbeat a "World += 1" program instead: the golden fixture
# tests/golden/tutorial3 was made that way, to exercise an effect on a per-object-callback
# property.)  "World" is
# added at runtime in the tutorial (NFCProperty defaults: not public, not private, so the AOI
# module sends it to nobody); SceneID / GroupID are private (IObject.xml), X / Y / Z public.
T3_INT_PROPS = ["SceneID", "GroupID", "World"]
T3_FLT_PROPS = ["X", "Y", "Z"]
T3_PROPS = T3_INT_PROPS + T3_FLT_PROPS
T3_PID = {n: i for i, n in enumerate(T3_PROPS)}
T3_KINDS = ["OnHeartBeat"]


def tutorial3_world(n_obj=10_000, n_ticks=120, tick_ms=100, seed=3, event_frac=0.01, t0=1_700_000_000_000,
                    guid_head=0, world_effect=False):
    rng = np.random.default_rng(seed)
    ni, nf = len(T3_INT_PROPS), len(T3_FLT_PROPS)
    # NFGUID(0, 10) in the tutorial; here NFGUID(guid_head, 10 + i)
    gdata = (10 + np.arange(n_obj)).astype(np.int64)
    ghead = np.full(n_obj, guid_head, np.int64)
    scene = np.ones(n_obj, np.int32)
    group = np.zeros(n_obj, np.int32)
    flags = np.zeros((1, len(T3_PROPS)), np.uint8)
    flags[0, T3_PID["SceneID"]] = PRIVATE
    flags[0, T3_PID["GroupID"]] = PRIVATE
    for n in ("X", "Y", "Z"):
        flags[0, T3_PID[n]] = PUBLIC | PRIVATE
    init_i = np.zeros((ni, n_obj), np.int64)
    init_i[T3_PID["SceneID"]] = 1
    init_i[T3_PID["World"]] = 1111   # pObject->SetPropertyInt("World", 1111) (:99)
    init_f = rng.uniform(-100.0, 100.0, (nf, n_obj))
    ops = np.zeros((1, MAX_OPS), OP_DTYPE)
    if world_effect:
        ops[0, 0] = (OP_IADD_CLAMP, 0, T3_PID["World"], 0, 1, I64_MIN, I64_MAX)
    n_ops = np.array([1 if world_effect else 0], np.int32)
    # objects created over the first 5 s (so the 5 s heartbeats do not all fire in one frame)
    s_time = (t0 - rng.integers(0, 5000, n_obj)).astype(np.int64)
    tick_time = (t0 + tick_ms * np.arange(1, n_ticks + 1)).astype(np.int64)
    # OnEvent -> SetPropertyInt(self, "World", arg.Int(0)) for a share of the objects every frame
    xt, xo, xb = [], [], []
    k = int(event_frac * n_obj)
    for t in range(n_ticks):
        if k:
            xt.append(np.full(k, t))
            xo.append(rng.integers(0, n_obj, k))
            xb.append(rng.integers(0, 1000, k).astype(np.uint64))
    cat = lambda lst, dt: np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
    x_tick, x_obj, x_bits = cat(xt, np.int32), cat(xo, np.int32), cat(xb, np.uint64)
    e32, e64, ef = np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return dict(
        cfg=np.array([n_obj, ni, nf, 1, 1, 0, n_obj, n_ticks], np.int64),
        prop_flags=flags, prop_names=_names(T3_PROPS), kind_names=_names(T3_KINDS), ops=ops, n_ops=n_ops,
        guid_head=ghead, guid_data=gdata, scene=scene, group=group, cls=np.zeros(n_obj, np.uint8),
        is_player=np.zeros(n_obj, np.uint8), init_i=init_i, init_f=init_f,
        s_obj=np.arange(n_obj, dtype=np.int32), s_kind=np.zeros(n_obj, np.int32),
        s_interval=np.full(n_obj, 5.0, np.float32), s_count=np.full(n_obj, 10, np.int32), s_time=s_time,
        tick_time=tick_time, x_tick=x_tick, x_obj=x_obj, x_pid=np.full(len(x_obj), T3_PID["World"], np.int32),
        x_bits=x_bits, h_tick=e32, h_op=e32, h_obj=e32, h_kind=e32, h_interval=ef, h_count=e32, h_time=e64,
        sw_tick=e32, sw_obj=e32, sw_scene=e32, sw_group=e32, sw_x=ef, sw_y=ef, sw_z=ef,
        scene_props=np.array([T3_PID["SceneID"], T3_PID["GroupID"], T3_PID["X"], T3_PID["Y"], T3_PID["Z"]],
                             np.int32))
