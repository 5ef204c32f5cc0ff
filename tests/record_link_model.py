"""Property links restated (test infrastructure): NFCPropertyModule::OnRecordPropertyEvent
(NFCPropertyModule.cpp:127-149) on a record of int columns, with the record calls that raise its events
(NFCRecord.cpp: AddRow :111-180, SetInt :182-235, GetInt :616-635, Remove / Clear :1086-1117,
SwapRowInfo :1219-1253).

LinkRecord is one object's record with a link (rows_l, col_pid[cols]).  Every call runs the
reference's steps in the reference's order and raises the record event at the reference's instant;
the event hands its nCol to the link:

    Update (an accepted set_int)        nCol = the cell's column, after the store
    Add / Cover (add_row)               nCol = 0, after the values are written and the row is used
    Del (remove, each step of clear)    nCol = 0, BEFORE the used bit is cleared
    Swap (swap_row_info)                nCol = the TARGET ROW's index, after the exchange

and the link, when nCol is a column with col_pid[nCol] >= 0, sets that property to the sum of column
nCol over rows [0, min(rows_l, rows)), GetInt being 0 for a row that is unused at that instant, each
cell truncated to int32 and the add taken modulo 2^32 (the device's rule; the reference's signed
int add is the same wherever it does not overflow), through SetPropertyInt's predicate: stored only
when different.  An nCol that is no column, or a column without a link, does nothing.

props: the object's int properties {pid: value}; sets: the accepted SetPropertyInt calls in order,
(pid, old, new).  frame_events() is what a frame reports for the window: per property one event from
the frame-start value to the final value, dropped when equal, in property-id order.
"""
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class LinkRecord:
    def __init__(self, rows, cols, rows_l=0, col_pid=None, props=None):
        self.rows, self.cols = int(rows), int(cols)
        self.rows_l = int(rows_l)
        self.col_pid = list(col_pid) if col_pid is not None else [-1] * self.cols
        assert len(self.col_pid) == self.cols
        self.used = 0
        self.cells = [[0] * self.rows for _ in range(self.cols)]   # [col][row], int64 values
        self.props = props if props is not None else {}
        self.start = {}         # pid -> value before the window's first accepted Set
        self.sets = []          # (pid, old, new) per accepted SetPropertyInt
        self.n_events = 0       # record events raised

    def is_used(self, row):
        return 0 <= row < self.rows and bool((self.used >> row) & 1)

    def get_int(self, row, col):
        if not (0 <= row < self.rows and 0 <= col < self.cols) or not self.is_used(row):
            return 0
        return self.cells[col][row]

    def link_sum(self, col):
        """the sum the link takes for column col now (a 32-bit int)"""
        s = 0
        for i in range(min(self.rows_l, self.rows)):
            s = (s + (self.get_int(i, col) & M32)) & M32
        return s32(s)

    def _event(self, ncol):
        self.n_events += 1
        if self.rows_l <= 0 or not (0 <= ncol < self.cols) or self.col_pid[ncol] < 0:
            return
        pid, v = self.col_pid[ncol], self.link_sum(ncol)
        old = self.props.get(pid, 0)
        if v != old:
            self.start.setdefault(pid, old)
            self.props[pid] = v
            self.sets.append((pid, old, v))

    # ---- the record calls ----
    def set_int(self, row, col, value):
        if not (0 <= row < self.rows and 0 <= col < self.cols) or not self.is_used(row):
            return False
        value = s64(value)
        if self.cells[col][row] == value:
            return False
        self.cells[col][row] = value
        self._event(col)
        return True

    def add_row(self, row, values=None):
        if row >= self.rows or (values is not None and len(values) != self.cols):
            return -1
        if row < 0:
            free = [r for r in range(self.rows) if not self.is_used(r)]
            if not free:
                return -1
            row = free[0]
        self.used |= 1 << row
        for c in range(self.cols):
            self.cells[c][row] = 0 if values is None else s64(values[c])
        self._event(0)
        return row

    def remove(self, row):
        if not self.is_used(row):
            return False
        self._event(0)
        self.used &= ~(1 << row)
        return True

    def clear(self):
        for row in range(self.rows - 1, -1, -1):
            self.remove(row)
        return True

    def swap_row_info(self, origin, target):
        if not self.is_used(origin) or not (0 <= target < self.rows):
            return False
        if origin != target:
            for c in range(self.cols):
                self.cells[c][origin], self.cells[c][target] = self.cells[c][target], self.cells[c][origin]
            ub = (self.used >> target) & 1
            self.used = (self.used & ~(1 << origin)) | (ub << origin) | (1 << target)
        self._event(target)
        return True

    # ---- the window ----
    def frame_events(self):
        """[(pid, frame-start value, final value)] in property-id order, equal ones dropped; the
        window's memory ends"""
        out = [(pid, old, self.props[pid]) for pid, old in sorted(self.start.items()) if old != self.props[pid]]
        self.start, self.sets = {}, []
        return out

    def apply(self, call):
        """one call as the tests write them: ("set", row, col, value), ("add", row, values or None),
        ("rm", row), ("clear",), ("swap", origin, target)"""
        k = call[0]
        if k == "set":
            return self.set_int(call[1], call[2], call[3])
        if k == "add":
            return self.add_row(call[1], call[2])
        if k == "rm":
            return self.remove(call[1])
        if k == "swap":
            return self.swap_row_info(call[1], call[2])
        return self.clear()


# values that meet equal cells often and reach the 32-bit edges
EDGE_VALUES = (0, 1, 2, 3, -1, 5, (1 << 32) + 5, -(1 << 31), (1 << 31) - 1, 1 << 31, -(1 << 63), (1 << 40) + 7)


def random_call(rng, rec):
    """one random call on `rec` (a LinkRecord): every kind, rows mostly low or the last one so that
    calls meet, swap targets often a column index"""
    rows, cols = rec.rows, rec.cols
    near = lambda: int(rng.choice([0, 1, 2, rows - 1])) % rows if rng.random() < 0.7 else int(rng.integers(0, rows))
    val = lambda: EDGE_VALUES[int(rng.integers(0, len(EDGE_VALUES)))] if rng.random() < 0.8 else int(rng.integers(-1000, 1000))
    k = int(rng.integers(0, 16))
    if k < 7:
        return ("set", near(), int(rng.integers(0, cols)), val())
    if k < 10:
        return ("swap", near(), near())
    if k < 12:
        return ("add", near(), [val() for _ in range(cols)])
    if k < 13:
        return ("add", -1, None)
    if k < 15:
        return ("rm", near())
    return ("clear",)


# ---- the golden world (tests/golden/record_link.json) ----
# The reference's Player with its CommPropertyValue record, 7 rows (the property groups NPG_JOBLEVEL ..
# NPG_RUNTIME_BUFF) x 16 int columns tagged with property names; tests/cpp/record_link_ref.cpp replays
# the script on the compiled NFCPropertyModule, replay() here.  The module's own calls:
#   SV / AV / UV <o> <group> <name> <v>   SetPropertyValue / AddPropertyValue / SubPropertyValue (PM:50-115):
#                                         SetUsed(group, true), then SetInt(group, name, an int value)
#   LV <o> <level> <v x cols>             Level Set -> RefreshBaseProperty (PM:117-125, 193-213): SetPropertyValue(tag,
#                                         NPG_JOBLEVEL, base value) for every column, in column order
# and the record's: SI / AR / RM / CL / SW (record_link_ref.cpp's header has the line formats).
GOLDEN_ROWS, GOLDEN_COLS = 7, 16
# (a tag that starts with "_" names no property: the reference's SetPropertyInt finds none, an unlinked column)
GOLDEN_TAGS = ["MAXHP", "MAXMP", "_NOPROP", "HPREGEN", "SPREGEN", "MPREGEN", "ATK_VALUE", "DEF_VALUE", "MOVE_SPEED",
               "ATK_SPEED", "ATK_FIRE", "ATK_LIGHT", "ATK_WIND", "ATK_ICE", "ATK_POISON", "DEF_FIRE"]
GOLDEN_BASE = [100 + 7 * c for c in range(GOLDEN_COLS)]
GOLDEN_OBJECTS = 8
GOLDEN_WINDOWS = 4
GOLDEN_SEED = 20261021


def set_used(rec, row):
    """NFCRecord::SetUsed(row, true): the bit, no event (the golden script only does it to used rows)"""
    if 0 <= row < rec.rows:
        rec.used |= 1 << row


def created(rows=GOLDEN_ROWS, cols=GOLDEN_COLS, base=GOLDEN_BASE, tags=GOLDEN_TAGS):
    """an object's record and properties right after NFCKernelModule::CreateObject: the module's class
    callback added every row (before it hooked the record, so no event) and set Level 1, whose
    callback wrote the base values into row 0 through the link"""
    r = LinkRecord(rows, cols, rows, [-1 if tags[c].startswith("_") else c for c in range(cols)],
                   props={c: 0 for c in range(cols)})
    r.used = (1 << rows) - 1
    for c in range(cols):
        r.set_int(0, c, base[c])
    r.frame_events()
    return r


def apply_line(rec, f, tags):
    """one call line on an object's LinkRecord -> the reference's return value"""
    op = f[0]
    if op in ("SV", "AV", "UV"):
        row, col, v = int(f[2]), tags.index(f[3]), s32(int(f[4]))
        set_used(rec, row)
        if op != "SV":
            cur = s32(rec.get_int(row, col))            # int nPropertyValue = pRecord->GetInt(...)
            v = s32(cur + v if op == "AV" else cur - v)
        return int(rec.set_int(row, col, v))
    if op == "SI":
        return int(rec.set_int(int(f[2]), int(f[3]), int(f[4])))
    if op == "AR":
        return rec.add_row(int(f[2]), [int(x) for x in f[3:]] if len(f) > 3 else None)
    if op == "RM":
        return int(rec.remove(int(f[2])))
    if op == "CL":
        return int(rec.clear())
    if op == "SW":
        return int(rec.swap_row_info(int(f[2]), int(f[3])))
    if op == "LV":
        for c in range(rec.cols):
            set_used(rec, 0)
            rec.set_int(0, c, s32(int(f[3 + c])))
        return 1
    raise ValueError(f)


def replay(script, on_call=None):
    """-> (the objects' values right after creation, [[ret, [the linked properties of the line's object]]]
    per call line)"""
    tags, base, objs, out = [], [], [], []
    for ln in script:
        f = ln.split()
        if f[0] == "SHAPE":
            rows, cols = int(f[1]), int(f[2])
        elif f[0] == "TAGS":
            tags = f[1:]
        elif f[0] == "BASE":
            base = [int(x) for x in f[1:]]
        elif f[0] == "OBJ":
            objs = [created(rows, cols, base, tags) for _ in range(int(f[1]))]
        elif f[0] == "X":
            if on_call:
                on_call(None, f, None)
        else:
            rec = objs[int(f[1])]
            if on_call:
                on_call(len(out), f, rec)
            ret = apply_line(rec, f, tags)
            out.append([int(ret), [rec.props[c] for c in range(rec.cols)]])
    # (right after creation every linked property is its base value; a column without a property reads 0)
    return [[0 if tags[c].startswith("_") else base[c] for c in range(len(tags))] for _ in objs], out


def golden_script(seed=GOLDEN_SEED):
    """The generator keeps the model beside the script so that a line meant as a case is one;
    count_conditions() counts the cases again from the replay."""
    import random
    rnd = random.Random(seed)
    rows, cols, tags = GOLDEN_ROWS, GOLDEN_COLS, GOLDEN_TAGS
    L = [f"SHAPE {rows} {cols}", "TAGS " + " ".join(tags), "BASE " + " ".join(str(v) for v in GOLDEN_BASE),
         f"OBJ {GOLDEN_OBJECTS}"]
    objs = [created() for _ in range(GOLDEN_OBJECTS)]

    def emit(ln):
        L.append(ln)
        f = ln.split()
        rec = objs[int(f[1])]
        apply_line(rec, f, tags)
        # every multi-term sum stays inside int32: the reference's add is a signed int add
        for c in range(cols):
            t = sum(s32(rec.cells[c][r]) for r in range(rows) if rec.is_used(r))
            assert -(1 << 31) <= t < (1 << 31), ln

    small = lambda: rnd.randrange(0, 400)
    tame = lambda rec: [(r, c) for r in range(rows) for c in range(cols) if rec.is_used(r) and abs(s32(rec.cells[c][r])) < 1 << 20]
    level = [1] * GOLDEN_OBJECTS
    for w in range(GOLDEN_WINDOWS):
        for o in rnd.sample(range(GOLDEN_OBJECTS), 5):
            rec = objs[o]
            used = lambda: [r for r in range(rows) if rec.is_used(r)]
            free = lambda: [r for r in range(rows) if not rec.is_used(r)]
            if not rec.is_used(0):
                emit(f"AR {o} 0 " + " ".join(str(small()) for _ in range(cols)))
            level[o] += 1 + rnd.randrange(3)                                     # a level-up
            emit(f"LV {o} {level[o]} " + " ".join(str(GOLDEN_BASE[c] + 11 * level[o] + c) for c in range(cols)))
            g = rnd.choice(used())
            c = rnd.randrange(cols)
            emit(f"SV {o} {g} {tags[c]} {small()}")                              # the module's calls, on used rows
            emit(f"SV {o} {g} {tags[c]} {s32(rec.get_int(g, c))}")               # an unchanged Set: no event
            r, c = rnd.choice(tame(rec))
            emit(f"AV {o} {r} {tags[c]} {rnd.randrange(1, 50)}")
            r, c = rnd.choice(tame(rec))
            emit(f"UV {o} {r} {tags[c]} {rnd.randrange(1, 50)}")
            r = rnd.choice([x for x in used() if x != 0] or used())
            emit(f"RM {o} {r}")                                                  # the removed row counted
            emit(f"SI {o} {r} {rnd.randrange(cols)} {small()}")                  # a Set on an unused row
            vals = [small() for _ in range(cols)]
            vals[rnd.randrange(1, cols)] = 777                                   # a stale property: a linked column other than 0
            emit(f"AR {o} {rnd.choice([-1, r])} " + " ".join(str(v) for v in vals))
            u = used()
            emit(f"SI {o} {rnd.choice(u)} {rnd.randrange(cols)} {(1 << 32) + 5}")
            # (-2^31 into a column that holds no other negative cell, so that its sum stays inside int32)
            ok = [c for c in range(cols) if all(s32(rec.cells[c][x]) >= 0 for x in u)]
            emit(f"SI {o} {rnd.choice(u)} {rnd.choice(ok)} {-(1 << 31)}")
            a, b = rnd.sample(u, 2) if len(u) > 1 else (u[0], u[0])
            emit(f"SW {o} {a} {b}")                                              # target: a column index < rows
            emit(f"SW {o} {rnd.choice(used())} 2")                               # target 2: the column without a property
            if free():
                emit(f"SW {o} {rnd.choice(used())} {free()[0]}")                 # a move
                emit(f"SW {o} {free()[0]} {rnd.choice(used())}")                 # origin unused: refused
            emit(f"AR {o} {rnd.choice(used())} " + " ".join(str(small()) for _ in range(cols)))   # Cover
            if rnd.random() < 0.3:
                emit(f"CL {o}")
                emit(f"AR {o} -1")
                emit(f"SV {o} 0 {tags[0]} {small()}")
        L.append("X")
    return L


CONDITIONS = ("unchanged Set", "Set on an unused row", "AddRow with a stale linked column", "Remove counts the removed row",
              "ClearRecord", "Swap to a linked column", "Swap to an unlinked column", "Swap refused", "cell 2^32 + 5", "cell -2^31", "level-up",
              "Add / Sub through the module", "Cover")


def count_conditions(script, answers):
    """how often each of CONDITIONS occurs, from the script replayed beside the answers.  (The record has
    fewer rows than columns, so a Swap's target row is always a column index: a target >= cols cannot
    occur in this world.)"""
    n = dict.fromkeys(CONDITIONS, 0)

    def watch(k, f, rec):
        if k is None:
            return
        op = f[0]
        ok = answers[k][0]
        if op in ("SV", "SI") and not ok:
            row = int(f[2])
            col = GOLDEN_TAGS.index(f[3]) if op == "SV" else int(f[3])
            if not rec.is_used(row):
                n["Set on an unused row"] += 1
            elif s64(int(f[4])) == rec.cells[col][row]:
                n["unchanged Set"] += 1
        if op == "SI" and ok and int(f[4]) == (1 << 32) + 5:
            n["cell 2^32 + 5"] += 1
        if op == "SI" and ok and int(f[4]) == -(1 << 31):
            n["cell -2^31"] += 1
        if op == "AR" and len(f) > 3 and any(int(v) != 0 for v in f[4:]) and ok >= 0:
            row = ok
            if any(int(f[3 + c]) != 0 and rec.col_pid[c] >= 0 for c in range(1, rec.cols)):
                n["AddRow with a stale linked column"] += 1
            if int(f[2]) >= 0 and rec.is_used(int(f[2])):
                n["Cover"] += 1
        if op == "RM" and ok and rec.cells[0][int(f[2])] != 0 and int(f[2]) < rec.rows_l:
            n["Remove counts the removed row"] += 1
        if op == "CL":
            n["ClearRecord"] += 1
        if op == "SW":
            n["Swap refused" if not ok else "Swap to a linked column" if rec.col_pid[int(f[3])] >= 0
              else "Swap to an unlinked column"] += 1
        if op == "LV":
            n["level-up"] += 1
        if op in ("AV", "UV") and ok:
            n["Add / Sub through the module"] += 1
    _, got = replay(script, watch)
    assert got == answers, "the model does not replay the answers"
    return n


def check_conditions(script, answers):
    n = count_conditions(script, answers)
    for name in CONDITIONS:
        assert n[name] >= 3, (name, n[name])
    return n
