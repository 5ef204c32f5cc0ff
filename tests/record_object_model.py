"""The reference's object (NFGUID) record columns restated over tests/record_find_model.Record (test
infrastructure).

ORecord is a record in the reference's LOGICAL columns, "I" (int64), "F" (f64) and "O" (NFGUID); its
cells are kept in the device's PHYSICAL layout, Record's [cols][rows] uint64 words, an object column
as two adjacent physical columns: the data half (nData64, type OBJ_DATA) at column c and the head
half (nHead64, OBJ_HEAD) at c + 1.  An NFGUID is a (head, data) pair of Python ints (int64 values).
NFCRecord::SetObject (RC:367), GetObject (RC:697), FindObject (RC:957), FindRowByColValue (RC:778)
and QueryRow (RC:554) are added to Record's calls, and every call logs the events the reference's
record hook receives: (op, row, logical col, old, new) with op 0 Update, 1 Add, 2 Del, 3 Cover (the
device's rrc op codes) and old / new as (head, data) pairs — an int / f64 cell's value is (0, bits),
a row event's (0, 0).

coalesce() is the per-window rule by which a frame's record events follow from the hook's: per
record the row events first, in call order, then one Update per cell in (row, col) order from the
first logged old value to the last logged new one, dropped when all 128 bits are equal.

golden_script() is the world of tests/golden/record_object.json: text lines that
tests/cpp/record_object_ref.cpp (the compiled reference) replays, and replay() here.
"""
import random

import numpy as np

from tests.record_find_model import FLOAT, INT, Record, f64_bits, i64_bits

OBJ_DATA, OBJ_HEAD = 2, 3           # NFK_REC_OBJ_DATA / NFK_REC_OBJ_HEAD
OBJECT = "O"                        # a FindRowByColValue var element's type, beside INT / FLOAT
EV_UPDATE, EV_ADD, EV_DEL, EV_COVER = 0, 1, 2, 3
NULL_OBJECT = (0, 0)
M64 = (1 << 64) - 1


def u64(x):
    return int(x) & M64


def s64(x):
    x = int(x) & M64
    return x - (1 << 64) if x >> 63 else x


def physical_types(logical):
    """'OIF' -> [2, 3, 0, 1]"""
    out = []
    for t in logical:
        out += [OBJ_DATA, OBJ_HEAD] if t == "O" else [FLOAT if t == "F" else INT]
    return out


class ORecord(Record):
    def __init__(self, rows, logical):
        self.logical = str(logical)
        super().__init__(rows, physical_types(self.logical))
        self.phys = []              # logical column -> physical column (an object's: its data half)
        c = 0
        for t in self.logical:
            self.phys.append(c)
            c += 2 if t == "O" else 1
        self.events = []            # the record hook's calls, in order

    @property
    def lcols(self):
        return len(self.logical)

    def _valid(self, row, col):
        return 0 <= row < self.rows and 0 <= col < self.lcols

    def words(self, values):
        """a row's logical values (ints as bit patterns, NFGUIDs as (head, data)) -> physical words"""
        out = []
        for t, v in zip(self.logical, values):
            out += [u64(v[1]), u64(v[0])] if t == "O" else [u64(v)]
        return out

    def _value(self, row, col):
        p = self.phys[col]
        if self.logical[col] == "O":
            return (s64(self.cells[p + 1, row]), s64(self.cells[p, row]))
        return (0, int(self.cells[p, row]))

    # ---- the row calls, with their events ----
    def add_row(self, row, values=None):
        """values: logical, one per column (None: the initial 0s / NULL_OBJECT)"""
        if values is not None and len(values) != self.lcols:
            return -1
        cover = row >= 0 and row < self.rows and self.is_used(row)
        got = super().add_row(row, None if values is None else self.words(values))
        if got >= 0:
            self.events.append((EV_COVER if cover else EV_ADD, got, 0, NULL_OBJECT, NULL_OBJECT))
        return got

    def remove(self, row):
        ok = super().remove(row)
        if ok:
            self.events.append((EV_DEL, row, 0, NULL_OBJECT, NULL_OBJECT))
        return ok

    def clear(self):
        for row in range(self.rows - 1, -1, -1):    # RC:1109: Remove from the last row to the first
            self.remove(row)
        return True

    def set_int(self, row, col, value):
        if not self._valid(row, col) or self.logical[col] != "I":
            return False
        old = self._value(row, col)
        ok = super().set_int(row, self.phys[col], value)
        if ok:
            self.events.append((EV_UPDATE, row, col, old, self._value(row, col)))
        return ok

    def set_object(self, row, col, value):
        """NFCRecord::SetObject (RC:367-421): refused on an invalid cell, a column of another type or
        an unused row; a value equal in both halves changes nothing and logs nothing"""
        if not self._valid(row, col) or self.logical[col] != "O" or not self.is_used(row):
            return False
        old = self._value(row, col)
        new = (s64(value[0]), s64(value[1]))
        if old == new:
            return False
        p = self.phys[col]
        self.cells[p, row] = u64(new[1])
        self.cells[p + 1, row] = u64(new[0])
        self.events.append((EV_UPDATE, row, col, old, new))
        return True

    # ---- reads and finds ----
    def get_object(self, row, col):
        if not self._valid(row, col) or self.logical[col] != "O" or not self.is_used(row):
            return NULL_OBJECT
        return self._value(row, col)

    def omask(self, col, value):
        """the rows FindObject finds as a bit mask (what nfk_find_objects returns)"""
        p = self.phys[col]
        used = np.array([self.is_used(r) for r in range(self.rows)], bool)
        eq = (self.cells[p] == np.uint64(u64(value[1]))) & (self.cells[p + 1] == np.uint64(u64(value[0])))
        return sum(1 << int(r) for r in np.nonzero(used & eq)[0])

    def find_object(self, col, value, result):
        if col < 0 or col >= self.lcols or self.logical[col] != "O":
            return -1
        m = self.omask(col, value)
        result.extend(r for r in range(self.rows) if (m >> r) & 1)
        return len(result)

    def find_int(self, col, value, result):
        if col < 0 or col >= self.lcols or self.logical[col] != "I":
            return -1
        return super().find_int(self.phys[col], value, result)

    def find_float(self, col, value, result):
        if col < 0 or col >= self.lcols or self.logical[col] != "F":
            return -1
        return super().find_float(self.phys[col], value, result)

    def find_row_by_col_value(self, col, var, result):
        """var: a list of (type, value), type INT / FLOAT / OBJECT.  var's element 0 gives the type,
        the value is read at index col (RC:778-822): 0 / 0.0 / NULL_OBJECT past var's end or for an
        element of another type."""
        if col < 0 or col >= self.lcols:
            return -1
        t0 = var[0][0] if var else None
        want = {"I": INT, "F": FLOAT, "O": OBJECT}[self.logical[col]]
        if t0 != want:
            return -1
        same = col < len(var) and var[col][0] == t0
        if t0 == OBJECT:
            return self.find_object(col, var[col][1] if same else NULL_OBJECT, result)
        v = var[col][1] if same else 0
        return self.find_int(col, v, result) if t0 == INT else self.find_float(col, v, result)

    def query_row(self, row):
        """the row's logical cells — ints / floats as bit patterns, NFGUIDs as (head, data) — or None"""
        if row < 0 or row >= self.rows or not self.is_used(row):
            return None
        return [self._value(row, c) if self.logical[c] == "O" else self._value(row, c)[1] for c in range(self.lcols)]


def coalesce(events):
    """one record's hook events of a window -> the frame's record events of it"""
    rows = [e for e in events if e[0] != EV_UPDATE]
    first, last = {}, {}
    for op, row, col, old, new in events:
        if op == EV_UPDATE:
            first.setdefault((row, col), old)
            last[(row, col)] = new
    cells = [(EV_UPDATE, row, col, first[(row, col)], last[(row, col)]) for row, col in sorted(first)
             if first[(row, col)] != last[(row, col)]]
    return rows + cells


# ---- the golden world: a script of text lines (tests/record_find_model.py's, with NFGUIDs) ----
#   REC <name> <rows> <types: I / F / O per logical column>     OBJ <n objects>
#   INIT <obj> <rec> <row> <values>          a creation-time row (before the first window)
#   SO <obj> <rec> <row> <col> <head:data>   SetObject         SI <obj> <rec> <row> <col> <int>   SetInt
#   RM <obj> <rec> <row>    AR <obj> <rec> <row | -1> [<values>]    CL <obj> <rec>    X  (the frame)
#   FO[+] <obj> <rec> <col> <head:data>      FindObject ("+": the list of the find before is kept)
#   FI[+] <obj> <rec> <col> <int>            FindInt
#   FV[+] <obj> <rec> <col> <n> <type> <value> ...   FindRowByColValue, types I / F / O
#   QR <obj> <rec> <row>                     QueryRow          GO <obj> <rec> <row> <col>   GetObject
# Columns are logical.  A value is an int in decimal, a float as C99 hex, an NFGUID as head:data.
# Every call line answers [ret, list, events]: ret the call's return value (a bool as 0 / 1; GO: 0),
# list the find's rows / QR's cells (an NFGUID as two entries, head then data; the others as uint64
# bit patterns) / GO's head and data, events the hook's calls it made as [op, row, col, old head, old
# data, new head, new data].
GOLDEN_RECORDS = [("Hero", 16, "OIF"), ("Team", 64, "O"), ("Pair", 5, "OO"), ("Edge", 20, "I" * 14 + "O")]
GOLDEN_OBJECTS = 24
GUIDS = [(3, 1001), (3, 1002), (4, 1001), (0, 7), (7, 0), (-1, -2), (3, 1 << 40)]
FLOATS = [0.0, 0.5, 1.5]


def _val(t, v):
    if t == "O":
        return f"{v[0]}:{v[1]}"
    return str(int(v)) if t == "I" else float(v).hex()


def golden_script():
    rnd = random.Random(20261021)
    L = [f"REC {n} {r} {t}" for n, r, t in GOLDEN_RECORDS] + [f"OBJ {GOLDEN_OBJECTS}"]
    rows_of = [r for _, r, _ in GOLDEN_RECORDS]
    types_of = [t for _, _, t in GOLDEN_RECORDS]
    ocols = [[c for c, t in enumerate(ts) if t == "O"] for ts in types_of]

    def guid():
        return rnd.choice(GUIDS)

    def values(rec):
        return " ".join(_val(t, guid() if t == "O" else rnd.randrange(0, 4) if t == "I" else rnd.choice(FLOATS))
                        for t in types_of[rec])

    for o in range(GOLDEN_OBJECTS):
        for rec in range(4):
            k = rnd.randrange(0, min(rows_of[rec], 8) + 1)
            rows = sorted(rnd.sample(range(rows_of[rec]), k))
            if rec == 1 and o % 5 == 0 and 63 not in rows:
                rows.append(63)
            for r in rows:
                L.append(f"INIT {o} {rec} {r} {values(rec)}")
    L.append("INIT 1 1 63 4:1001")    # the find that hits row 63

    def finds(objs):
        for o in objs:
            rec = rnd.randrange(4)
            L.append(f"FO {o} {rec} {rnd.choice(ocols[rec])} {_val('O', guid())}")
            rec = rnd.randrange(4)
            L.append(f"FO {o} {rec} {rnd.choice(ocols[rec])} {_val('O', guid())}")
            L.append(f"GO {o} {rec} {rnd.randrange(rows_of[rec])} {rnd.choice(ocols[rec])}")
        o = objs[0]
        L.append(f"QR {o} 0 {rnd.randrange(16)}")
        L.append(f"QR {o} 3 {rnd.randrange(20)}")
        L.append(f"QR {o} 1 63")

    for t in range(4):
        touched = rnd.sample(range(GOLDEN_OBJECTS), 8)
        for o in touched[:6]:
            rec = rnd.randrange(4)
            L.append(f"SO {o} {rec} {rnd.randrange(rows_of[rec])} {rnd.choice(ocols[rec])} {_val('O', guid())}")
            L.append(f"SO {o} 0 {rnd.randrange(16)} 0 {_val('O', guid())}")
            L.append(f"SI {o} 0 {rnd.randrange(16)} 1 {rnd.randrange(0, 4)}")
            L.append(f"RM {o} {rnd.randrange(4)} {rnd.randrange(5)}")
            L.append(f"AR {o} 0 -1")
            L.append(f"AR {o} 0 {rnd.randrange(16)} {values(0)}")
            L.append(f"AR {o} 1 {rnd.choice([63, rnd.randrange(64)])} {values(1)}")
            L.append(f"AR {o} 2 {rnd.randrange(5)} {values(2)}")
            L.append(f"AR {o} 3 {rnd.randrange(20)} {values(3)}")
            L.append(f"SO {o} 3 {rnd.randrange(20)} 14 {_val('O', guid())}")
            L.append(f"SO {o} 2 {rnd.randrange(5)} {rnd.randrange(2)} {_val('O', guid())}")
        L.append(f"CL {touched[6]} 0")
        L.append(f"CL {touched[7]} 1")
        L.append(f"AR {touched[7]} 1 -1")
        o = touched[0]
        # a removed row's stale NFGUID is not found; the row re-added without values holds NULL_OBJECT
        L += [f"AR {o} 0 5 3:1001 3 0x1.8p+0", f"RM {o} 0 5", f"FO {o} 0 0 3:1001", f"SO {o} 0 5 0 4:1001",
              f"AR {o} 0 5", f"FO {o} 0 0 0:0", f"FO {o} 0 0 3:1001", f"QR {o} 0 5", f"GO {o} 0 5 0"]
        # an equal value; only the head half changes, then only the data half; away and back in one window
        L += [f"AR {o} 2 1 3:1001 3:1002", f"SO {o} 2 1 0 3:1001", f"SO {o} 2 1 0 4:1001", f"SO {o} 2 1 0 4:1002",
              f"SO {o} 2 1 1 7:0", f"SO {o} 2 1 1 3:1002", f"GO {o} 2 1 0", f"GO {o} 2 1 1", f"FO {o} 2 0 4:1002",
              f"FO {o} 2 0 4:1001", f"FO {o} 2 0 3:1002"]
        others = [x for x in range(GOLDEN_OBJECTS) if x not in touched]
        finds(touched[:4] + rnd.sample(others, 4))               # mid-window
        L += [f"FO {touched[1]} 0 0 3:1001", f"FO+ {touched[1]} 0 0 3:1002", f"FI+ {touched[1]} 0 1 2"]
        # FindRowByColValue: var's element 0 gives the type, element nCol the value
        L += [f"FV {others[1]} 0 0 1 O 3:1001", f"FV {others[1]} 2 1 2 O 3:1001 O 3:1002", f"FV {others[1]} 2 1 1 O 3:1001",
              f"FV {others[1]} 2 1 2 O 3:1001 I 5", f"FV {others[1]} 0 0 1 I 3", f"FV {others[1]} 0 1 1 O 3:1001",
              f"FV {others[1]} 3 14 1 O 3:1001", f"FV {others[1]} 0 1 2 I 9 I 2", f"FV {others[1]} 0 0 0"]
        # -1 / false: a column of another type, a column outside the record, an unknown record / object
        L += [f"FO {others[2]} 0 1 3:1001", f"FI {others[2]} 0 0 3", f"FO {others[2]} 0 3 3:1001", f"FO {others[2]} 0 -1 3:1001",
              f"FO {others[2]} 4 0 3:1001", f"FO {GOLDEN_OBJECTS} 0 0 3:1001", f"SO {others[2]} 0 0 1 3:1001",
              f"SI {others[2]} 0 0 0 3", f"SO {others[2]} 0 16 0 3:1001", f"GO {others[2]} 0 0 1"]
        L.append("X")
        finds(touched[:4] + rnd.sample(others, 4))               # after the frame applied the calls
        L += [f"FO {touched[0]} 0 0 0:0", f"QR {touched[0]} 0 5", f"FO {touched[7]} 1 0 0:0", f"GO {touched[0]} 2 1 0"]
        if t == 0:
            L += ["FO 1 1 0 4:1001", "QR 1 1 63", "GO 1 1 63 0"]
    return L


def parse_guid(tok):
    h, d = tok.split(":")
    return (int(h), int(d))


def parse_values(tok, types):
    return [parse_guid(v) if t == "O" else i64_bits(int(v)) if t == "I" else f64_bits(float.fromhex(v))
            for t, v in zip(types, tok)]


def parse_var(f):
    """the FV line's var (from field 4 on) -> [(type, value)]"""
    var = []
    for k in range(int(f[4])):
        t, v = f[5 + 2 * k], f[6 + 2 * k]
        var.append((OBJECT, parse_guid(v)) if t == "O" else (INT, int(v)) if t == "I" else (FLOAT, float.fromhex(v)))
    return var


def flat_event(e):
    op, row, col, old, new = e
    return [op, row, col, u64(old[0]), u64(old[1]), u64(new[0]), u64(new[1])]   # (uint64 bit patterns)


def flat_row(q):
    out = []
    for v in q:
        out += [u64(v[0]), u64(v[1])] if isinstance(v, tuple) else [int(v)]
    return out


def replay(script, on_call=None):
    """the script's answers by the model: [ret, list, events] per call line, in order.  on_call(k,
    line, fields, objs): called before call k is applied (objs[o][r]: the ORecords), for a test that
    drives a device beside the model."""
    defs, objs, out, last = [], [], [], []
    for ln in script:
        f = ln.split()
        op = f[0]
        if op == "REC":
            defs.append((int(f[2]), f[3]))
            continue
        if op == "OBJ":
            objs = [[ORecord(r, t) for r, t in defs] for _ in range(int(f[1]))]
            continue
        if op == "X":
            if on_call:
                on_call(None, ln, f, objs)
            continue
        if on_call:
            on_call(len(out), ln, f, objs)
        o, r = int(f[1]), int(f[2])
        known = 0 <= o < len(objs) and 0 <= r < len(defs)
        rec = objs[o][r] if known else None
        n0 = len(rec.events) if known else 0
        ret, lst = 0, []
        if op in ("INIT", "AR"):
            ret = rec.add_row(int(f[3]), parse_values(f[4:], rec.logical) if len(f) > 4 else None) if known else -1
        elif op == "SO":
            ret = int(known and rec.set_object(int(f[3]), int(f[4]), parse_guid(f[5])))
        elif op == "SI":
            ret = int(known and rec.set_int(int(f[3]), int(f[4]), int(f[5])))
        elif op == "RM":
            ret = int(known and rec.remove(int(f[3])))
        elif op == "CL":
            ret = int(known and rec.clear())
        elif op == "QR":
            q = rec.query_row(int(f[3])) if known else None
            ret, lst = (0 if q is None else 1), flat_row(q or [])
        elif op == "GO":
            g = rec.get_object(int(f[3]), int(f[4])) if known else NULL_OBJECT
            lst = [u64(g[0]), u64(g[1])]
        else:
            if not op.endswith("+"):
                last = []
            col = int(f[3])
            if not known:
                ret = -1
            elif op[:2] == "FO":
                ret = rec.find_object(col, parse_guid(f[4]), last)
            elif op[:2] == "FI":
                ret = rec.find_int(col, int(f[4]), last)
            else:
                ret = rec.find_row_by_col_value(col, parse_var(f), last)
            lst = list(last)
        ev = [flat_event(e) for e in rec.events[n0:]] if known else []
        out.append([int(ret), lst, ev])
    return out


def check_conditions(script, answers):
    """what the golden is there for (the generator asserts it, tests/test_record_object.py again)"""
    calls = [ln for ln in script if ln.split()[0] not in ("REC", "OBJ", "X")]
    assert len(calls) == len(answers)
    ca = [(c.split(), a) for c, a in zip(calls, answers)]
    finds = [(c, a) for c, a in ca if c[0][0] == "F"]
    assert sum(1 for c, a in finds if a[1]) >= 30, "finds with a hit"
    assert sum(1 for c, a in finds if len(a[1]) > 1) >= 5, "finds with more than one row"
    assert sum(1 for c, a in finds if a[0] == -1) >= 3, "finds returning -1"
    assert any(63 in a[1] for c, a in finds), "a hit on row 63"
    # a find of NULL_OBJECT that hits a row re-added without values: `AR o r row` directly before it
    hit = False
    for i in range(len(ca) - 1):
        c, (n, nxt) = ca[i][0], ca[i + 1]
        if c[0] == "AR" and len(c) == 4 and n[0] == "FO" and n[1:3] == c[1:3] and n[4] == "0:0":
            hit = hit or int(c[3]) in nxt[1]
    assert hit, "a find of NULL_OBJECT that hits a re-added row"
    sos = [(c, a) for c, a in ca if c[0] == "SO"]
    # refused on an unused row: a valid object cell, return 0, while the row is not used (replayed)
    st = {"unused": False}

    def watch(k, ln, f, objs):
        if k is not None and f[0] == "SO" and answers[k][0] == 0:
            o, r = int(f[1]), int(f[2])
            if o < len(objs) and r < len(objs[o]):
                rec = objs[o][r]
                row, col = int(f[3]), int(f[4])
                if rec._valid(row, col) and rec.logical[col] == "O" and not rec.is_used(row):
                    st["unused"] = True
    replay(script, watch)
    assert st["unused"], "a SetObject refused on an unused row"
    upd = [a[2][0] for c, a in sos if a[0] == 1 and a[2]]
    assert any(a[0] == 0 and not a[2] for c, a in sos), "a SetObject returning false"
    assert any(e[3] != e[5] and e[4] == e[6] for e in upd), "a SetObject changing only the head half"
    assert any(e[3] == e[5] and e[4] != e[6] for e in upd), "a SetObject changing only the data half"
    # a cell set away and back within one window: its Updates coalesce to nothing
    cells, k, back = {}, 0, False
    for ln in script:
        f = ln.split()
        if f[0] in ("REC", "OBJ"):
            continue
        if f[0] == "X":
            cells = {}
            continue
        for e in answers[k][2]:
            if e[0] == EV_UPDATE and f[0] == "SO":
                c = cells.setdefault((f[1], f[2], e[1], e[2]), [tuple(e[3:5]), None, 0])
                c[1], c[2] = tuple(e[5:7]), c[2] + 1
                back = back or (c[2] >= 2 and c[0] == c[1])
        k += 1
    assert back, "a cell set away and back within one window"
    # equal value: false on a used row whose cell holds the value (the script's `SO o 2 1 0 3:1001`)
    assert any(c[1:] == ca[i - 1][0][1:4] + ["0", ca[i - 1][0][4]] and a[0] == 0
               for i, (c, a) in enumerate(ca) if i and c[0] == "SO" and ca[i - 1][0][0] == "AR"
               and len(ca[i - 1][0]) > 4), "a SetObject returning false for an equal value"
