"""Resource calls restated (test infrastructure): the spending half of NFCPropertyModule
(NFCPropertyModule.cpp:215-472) — FullHPMP, FullSP, Add / Consume / Enough of HP, MP, SP, Money and
Diamond — as seven rules over a dict world {(object, property): int64}.

    rule(op, cur, mx, v) -> (the reference's return value, the value it Sets or None)
    adjust(world, calls) -> (result bytes, the Sets in call order); calls: (object, op, dst, bound, v)

A call reads the world as the calls before it left it; add and subtract wrap at 64 bits (the
device's rule; signed overflow is undefined in the reference, and the golden script has none).

The golden world (tests/golden/resource_calls.json): the reference's Player with HP, MP, SP, Gold,
Money and the three maxima MAXHP, MAXMP, MAXSP as the columns of its CommPropertyValue record, so the
maxima move through the module's own link (PM:127-149: the int sum of the column over the seven
property groups).  tests/cpp/resource_calls_ref.cpp replays golden_script() on the compiled module,
replay() here.
"""
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

GAIN_ALIVE, GAIN_CAP, GAIN, SPEND_ALIVE, SPEND, ENOUGH, FILL = range(7)
TAKES_BOUND = (GAIN_ALIVE, GAIN_CAP, FILL)
RET, SET = 1, 2


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def rule(op, cur, mx, v):
    """one call on the value cur (and the maximum mx): (return value, new value or None)"""
    if op == GAIN_ALIVE:                     # AddHP PM:232
        if v <= 0:
            return 0, None
        if cur <= 0:
            return 1, None
        return 1, min(s64(cur + v), mx)
    if op == GAIN_CAP:                       # AddMP / AddSP PM:281, 340
        if v <= 0:
            return 0, None
        return 1, min(s64(cur + v), mx)
    if op == GAIN:                           # AddMoney / AddDiamond PM:386, 430: false on both branches
        if v <= 0:
            return 0, None
        return 0, s64(cur + v)
    if op == SPEND_ALIVE:                    # ConsumeHP / MP / SP PM:267, 302, 361: v is not tested
        if cur > 0 and s64(cur - v) >= 0:
            return 1, s64(cur - v)
        return 0, None
    if op == SPEND:                          # ConsumeMoney / ConsumeDiamond PM:400, 444
        if v <= 0:
            return 0, None
        n = s64(cur - v)
        return (1, n) if n >= 0 else (0, None)
    if op == ENOUGH:                         # every Enough* PM:256...
        return int(cur > 0 and s64(cur - v) >= 0), None
    if op == FILL:                           # FullSP, each half of FullHPMP PM:215, 327
        return (1, mx) if mx > 0 else (0, None)
    raise ValueError(op)


def adjust(world, calls):
    """the batch applied in order on world {(object, pid): value} (a missing cell reads 0) ->
    ([result byte per call], [(object, dst, new) per Set])"""
    rets, sets = [], []
    for o, op, dst, bound, v in calls:
        cur = world.get((o, dst), 0)
        mx = world.get((o, bound), 0) if bound >= 0 else 0
        r, nv = rule(op, cur, mx, s64(v))
        if nv is not None:
            world[(o, dst)] = nv
            sets.append((o, dst, nv))
            r |= SET
        rets.append(r)
    return rets, sets


# ---- NFIPropertyModule's seventeen names: the calls each makes, (op, dst, bound) by property name ----
PROPS = ["HP", "MP", "SP", "MAXHP", "MAXMP", "MAXSP", "Gold", "Money"]
METHODS = {
    "AddHP": [(GAIN_ALIVE, "HP", "MAXHP")], "ConsumeHP": [(SPEND_ALIVE, "HP", None)], "EnoughHP": [(ENOUGH, "HP", None)],
    "AddMP": [(GAIN_CAP, "MP", "MAXMP")], "ConsumeMP": [(SPEND_ALIVE, "MP", None)], "EnoughMP": [(ENOUGH, "MP", None)],
    "AddSP": [(GAIN_CAP, "SP", "MAXSP")], "ConsumeSP": [(SPEND_ALIVE, "SP", None)], "EnoughSP": [(ENOUGH, "SP", None)],
    "FullHPMP": [(FILL, "HP", "MAXHP"), (FILL, "MP", "MAXMP")], "FullSP": [(FILL, "SP", "MAXSP")],
    "AddMoney": [(GAIN, "Gold", None)], "ConsumeMoney": [(SPEND, "Gold", None)], "EnoughMoney": [(ENOUGH, "Gold", None)],
    "AddDiamond": [(GAIN, "Money", None)], "ConsumeDiamond": [(SPEND, "Money", None)],
    "EnoughDiamond": [(ENOUGH, "Money", None)],
}
TWO_RETURNS = [m for m in METHODS if m not in ("FullHPMP", "AddMoney", "AddDiamond")]   # (the others answer one value only)


def method_calls(name, o, v, pid=PROPS.index):
    """the (object, op, dst, bound, v) calls of one named method"""
    return [(o, op, pid(d), -1 if b is None else pid(b), v) for op, d, b in METHODS[name]]


def method_return(name, rets):
    """the method's bool from its calls' result bytes (FullHPMP answers true whatever they say)"""
    return 1 if name == "FullHPMP" else rets[-1] & RET


# ---- the golden world ----
GROUPS = 7                       # NPG_JOBLEVEL .. NPG_RUNTIME_BUFF: the rows the link sums
LINK_TAGS = ["MAXHP", "MAXMP", "MAXSP"]
GOLDEN_BASE = [100, 50, 30]
GOLDEN_OBJECTS = 5
NOBODY = 99                      # an object index whose NFGUID nobody has


class Player:
    """one object of the golden world: the eight properties and the CommPropertyValue cells"""

    def __init__(self, base):
        self.props = dict.fromkeys(PROPS, 0)
        self.cells = [[0] * GROUPS for _ in LINK_TAGS]   # [col][group]
        self.level = 0
        self.set_level(1, base)

    def world(self):
        return {(0, i): self.props[n] for i, n in enumerate(PROPS)}

    def call(self, name, v):
        w = self.world()
        rets, _ = adjust(w, method_calls(name, 0, v))
        for i, n in enumerate(PROPS):
            self.props[n] = w[(0, i)]
        return method_return(name, rets)

    def set_value(self, group, tag, v):
        """SetPropertyValue(tag, group, int v) (PM:50): the record's SetInt; an accepted one raises
        the event that sums the column into the property"""
        c, v = LINK_TAGS.index(tag), s32(v)
        if self.cells[c][group] == v:
            return 0
        self.cells[c][group] = v
        self.props[tag] = s32(sum(self.cells[c]))
        return 1

    def set_level(self, level, base):
        """SetPropertyInt(Level): the level callback (PM:117) rewrites the base values, then fills"""
        if level == self.level:
            return 1
        self.level = level
        for c, tag in enumerate(LINK_TAGS):
            self.set_value(0, tag, base[c])
        self.call("FullHPMP", 0)
        self.call("FullSP", 0)
        return 1


def apply_line(objs, f):
    """one call line -> the reference's return value"""
    o = int(f[1])
    if f[0] in METHODS:
        v = int(f[2]) if len(f) > 2 else 0
        if o not in objs:      # GetPropertyInt answers 0 and the Set is dropped: the rules on a world of zeros
            return method_return(f[0], adjust({}, method_calls(f[0], 0, v))[0])
        return objs[o].call(f[0], v)
    p = objs[o]
    if f[0] == "SV":
        return p.set_value(int(f[2]), f[3], int(f[4]))
    if f[0] == "LV":
        return p.set_level(int(f[2]), [int(x) for x in f[3:6]])
    if f[0] == "SP":           # NFCKernelModule::SetPropertyInt of an unlinked property
        assert f[2] not in LINK_TAGS
        p.props[f[2]] = s64(int(f[3]))
        return 1
    raise ValueError(f)


def replay(script, on_call=None):
    """-> [[ret, [the line's object's eight properties after the call]]] per call line; on_call(k, f,
    player or None, the properties before) sees every call line first"""
    objs, out, base = {}, [], GOLDEN_BASE
    for ln in script:
        f = ln.split()
        if f[0] == "BASE":
            base = [int(x) for x in f[1:]]
        elif f[0] == "OBJ":
            objs = {o: Player(base) for o in range(int(f[1]))}
        elif f[0] == "X":
            continue
        else:
            p = objs.get(int(f[1]))
            if on_call:
                on_call(len(out), f, p, dict(p.props) if p else dict.fromkeys(PROPS, 0))
            ret = apply_line(objs, f)
            out.append([int(ret), [p.props[n] if p else 0 for n in PROPS]])
    return out


def golden_script():
    """written by hand, case by case; check_conditions() finds the cases again in the answers"""
    B = 1 << 33
    L = ["BASE " + " ".join(str(v) for v in GOLDEN_BASE), f"OBJ {GOLDEN_OBJECTS}"]
    # object 0: HP, mid-window chains (created at HP 100 / 100, MP 50 / 50, SP 30 / 30)
    L += ["ConsumeHP 0 40", "AddHP 0 10", "AddHP 0 500",           # 60, 70, then exactly MAXHP
          "AddHP 0 0", "AddHP 0 -5", "EnoughHP 0 100", "EnoughHP 0 101",
          "ConsumeHP 0 101", "ConsumeHP 0 100",                   # one past 0: refused; then exactly 0
          "AddHP 0 5", "EnoughHP 0 0", "ConsumeHP 0 0",           # HP == 0: nothing, false, false
          "X",
          "FullHPMP 0", "SV 0 3 MAXHP -60", "AddHP 0 1",          # MAXHP 40 < HP 100: AddHP lowers HP
          "ConsumeHP 0 -1000", f"ConsumeHP 0 {-B}",               # a negative value raises HP past MAXHP
          "AddHP 0 1", "X"]
    # object 1: MP and SP
    L += ["ConsumeMP 1 50", "ConsumeMP 1 1", "EnoughMP 1 0",      # exactly 0; then refused
          "AddMP 1 7", "AddMP 1 0", "AddMP 1 1000",               # MP == 0 is raised, unlike HP; capped
          "ConsumeMP 1 51", "EnoughMP 1 50", "EnoughMP 1 51", "ConsumeMP 1 20", "X",
          "ConsumeSP 1 30", "ConsumeSP 1 1", "AddSP 1 4", "AddSP 1 -1", "AddSP 1 99", "EnoughSP 1 30", "EnoughSP 1 31",
          "ConsumeSP 1 31", "ConsumeSP 1 29", "FullSP 1",
          "SV 1 0 MAXSP 0", "FullSP 1", "AddSP 1 5",              # MAXSP 0: FullSP false, AddSP caps SP at 0
          "X"]
    # object 2: Gold and Money, values beyond 2^32
    L += ["EnoughMoney 2 0", "ConsumeMoney 2 1", "AddMoney 2 -1", "AddMoney 2 0", "ConsumeMoney 2 0",
          f"AddMoney 2 {B + 7}", "AddMoney 2 3", "ConsumeMoney 2 0", "AddMoney 2 -1", f"EnoughMoney 2 {B + 10}", f"EnoughMoney 2 {B + 11}",
          f"ConsumeMoney 2 {B + 11}", "ConsumeMoney 2 10", f"ConsumeMoney 2 {B}", "EnoughMoney 2 0", "X",
          "EnoughDiamond 2 1", "AddDiamond 2 -3", f"AddDiamond 2 {3 * B}", f"ConsumeDiamond 2 {B}", "ConsumeDiamond 2 -1",
          f"EnoughDiamond 2 {2 * B}", f"EnoughDiamond 2 {2 * B + 1}", f"ConsumeDiamond 2 {2 * B + 1}",
          f"ConsumeDiamond 2 {2 * B}", "ConsumeDiamond 2 1", "X"]
    # object 3: the maxima move between two calls (SetPropertyValue, a level callback), MAXMP == 0
    L += ["ConsumeHP 3 90", "AddHP 3 500", "SV 3 2 MAXHP 150", "AddHP 3 500",        # 100, then 250
          "SV 3 0 MAXMP 0", "ConsumeMP 3 45", "ConsumeHP 3 200", "FullHPMP 3",       # MAXMP 0: HP filled, MP left alone
          "AddMP 3 3", "X",
          "LV 3 2 120 60 40", "ConsumeHP 3 100", "AddHP 3 1000", "FullSP 3",         # the callback fills at the new maxima
          "SP 3 HP 0", "FullHPMP 3", "SP 3 Gold 5", "ConsumeMoney 3 5", "X"]
    # object 4: untouched until now, then one call of every method back to back
    L += [f"{m} 4 3" if m not in ("FullHPMP", "FullSP") else f"{m} 4" for m in METHODS]
    L += ["X"]
    # an NFGUID nobody has
    L += [f"{m} {NOBODY} 3" if m not in ("FullHPMP", "FullSP") else f"{m} {NOBODY}" for m in METHODS]
    L += ["X"]
    return L


CONDITIONS = (
    "every method, both return values", "AddHP on HP == 0", "AddHP reaches exactly MAXHP", "AddHP with MAXHP < HP lowers HP",
    "AddMP on MP == 0 raises it", "Consume to exactly 0", "Consume one past 0", "ConsumeHP with a negative value passes MAXHP",
    "ConsumeMoney(0)", "AddMoney(-1)", "EnoughMoney(0) on Gold == 0", "FullHPMP with MAXMP == 0",
    "a maximum changed between two calls", "two calls on one object back to back", "an NFGUID nobody has", "values beyond 2^32")


def count_conditions(script, answers):
    """how often each of CONDITIONS occurs in the reference's answers (the model replays beside
    them to know each call's state before)"""
    n = dict.fromkeys(CONDITIONS, 0)
    seen = {}          # method -> the return values it gave
    last = [None]      # the previous call line: (object, was a method, was a change of a maximum)
    before_max = {}

    def watch(k, f, p, before):
        ret, after = answers[k][0], dict(zip(PROPS, answers[k][1]))
        m, o = f[0], int(f[1])
        v = int(f[2]) if m in METHODS and len(f) > 2 else 0
        if m in METHODS:
            seen.setdefault(m, set()).add(ret)
            if p is None:
                n["an NFGUID nobody has"] += 1
            elif last[0] == (o, True):
                n["two calls on one object back to back"] += 1
            if p is not None and before_max.get(o) is not None and METHODS[m][0][2] is not None:
                if before_max[o] != [before[t] for t in LINK_TAGS]:
                    n["a maximum changed between two calls"] += 1
            if p is not None:
                before_max[o] = [before[t] for t in LINK_TAGS]
            if any(abs(x) > 1 << 32 for x in [v] + list(after.values())):
                n["values beyond 2^32"] += 1
        if p is not None:
            if m == "AddHP" and v > 0 and before["HP"] == 0 and ret == 1 and after["HP"] == 0:
                n["AddHP on HP == 0"] += 1
            if m == "AddHP" and 0 < before["HP"] < before["MAXHP"] == after["HP"]:
                n["AddHP reaches exactly MAXHP"] += 1
            if m == "AddHP" and v > 0 and before["MAXHP"] < before["HP"] and after["HP"] < before["HP"]:
                n["AddHP with MAXHP < HP lowers HP"] += 1
            if m == "AddMP" and before["MP"] == 0 and after["MP"] > 0:
                n["AddMP on MP == 0 raises it"] += 1
            if m.startswith("Consume"):
                d = METHODS[m][0][1]
                if ret and before[d] > 0 and after[d] == 0:
                    n["Consume to exactly 0"] += 1
                if not ret and v == before[d] + 1 and after[d] == before[d] > 0:
                    n["Consume one past 0"] += 1
            if m == "ConsumeHP" and v < 0 and ret and after["HP"] > after["MAXHP"]:
                n["ConsumeHP with a negative value passes MAXHP"] += 1
            if m == "ConsumeMoney" and v == 0 and not ret and before["Gold"] > 0:
                n["ConsumeMoney(0)"] += 1
            if m == "AddMoney" and v == -1 and not ret and after["Gold"] == before["Gold"]:
                n["AddMoney(-1)"] += 1
            if m == "EnoughMoney" and v == 0 and before["Gold"] == 0 and not ret:
                n["EnoughMoney(0) on Gold == 0"] += 1
            if m == "FullHPMP" and before["MAXMP"] == 0 and before["HP"] != before["MAXHP"] == after["HP"] \
                    and after["MP"] == before["MP"] != 0:
                n["FullHPMP with MAXMP == 0"] += 1
        last[0] = (o, m in METHODS)
    got = replay(script, watch)
    assert got == answers, "the model does not replay the answers"
    n["every method, both return values"] = sum(
        1 for m in METHODS if seen.get(m, set()) >= ({0, 1} if m in TWO_RETURNS else {1 if m == "FullHPMP" else 0}))
    return n


def check_conditions(script, answers):
    n = count_conditions(script, answers)
    for name in CONDITIONS:
        assert n[name] >= (len(METHODS) if name == "every method, both return values" else 1), (name, n[name])
    return n
