"""The reference's record finds restated in numpy (test infrastructure).

NFCRecord::FindInt (RC:830), FindFloat (RC:873), FindRowByColValue (RC:778) and QueryRow (RC:554)
over one record's state: its used-row mask (bit r: row r is used), its cells as uint64 bit patterns
[cols][rows] in ROW order and its column types (0 int64, 1 f64) — with the row calls the finds are
asked between: AddRow (RC:111), Remove (RC:1086, the cells keep their values), Clear (RC:1109) and
SetInt (RC:182).  Lists are Python lists of rows that the calls APPEND to, as the reference's
`varResult << i`; the return value is the list's total size (RC:856).

golden_script() is the world of tests/golden/record_find.json: a list of text lines that
tests/cpp/record_find_ref.cpp (the compiled reference) and tests/cpp/record_find_plugin.cpp (the C++
plugin on a GPU) both replay, and replay() here.
"""
import random

import numpy as np

INT, FLOAT = 0, 1


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


def i64_bits(x):
    return int(np.int64(x).view(np.uint64))


class Record:
    def __init__(self, rows, col_types, used=0, cells=None):
        self.rows = int(rows)
        self.types = [int(t) for t in col_types]
        self.used = int(used)
        self.cells = (np.zeros((len(self.types), self.rows), np.uint64) if cells is None
                      else np.array(cells, np.uint64).reshape(len(self.types), self.rows))

    @property
    def cols(self):
        return len(self.types)

    def is_used(self, row):
        return bool((self.used >> row) & 1)

    # ---- the row calls ----
    def add_row(self, row, values=None):
        """AddRow(row) / AddRow(row, values): values as uint64 bit patterns [cols]; None: the
        columns' initial 0s (RC:106).  Returns the row taken, or -1."""
        if row >= self.rows:
            return -1
        if values is not None and len(values) != self.cols:
            return -1
        if row < 0:
            free = [r for r in range(self.rows) if not self.is_used(r)]
            if not free:
                return -1
            row = free[0]
        self.used |= 1 << row
        for c in range(self.cols):
            self.cells[c, row] = 0 if values is None else values[c]
        return row

    def remove(self, row):
        if row < 0 or row >= self.rows or not self.is_used(row):
            return False
        self.used &= ~(1 << row)   # (the cells stay: RC:1086-1107)
        return True

    def clear(self):
        self.used = 0

    def set_int(self, row, col, value):
        if row < 0 or row >= self.rows or col < 0 or col >= self.cols or self.types[col] != INT:
            return False
        if not self.is_used(row) or int(self.cells[col, row]) == i64_bits(value):
            return False
        self.cells[col, row] = i64_bits(value)
        return True

    # ---- the finds ----
    def mask(self, col, bits):
        """the rows found as a bit mask: used rows whose cell equals `bits` under the column's type
        (what nfk_find_rows returns)"""
        used = np.array([self.is_used(r) for r in range(self.rows)], bool)
        c = self.cells[col]
        if self.types[col] == FLOAT:
            with np.errstate(invalid="ignore"):
                eq = c.view(np.float64) == np.uint64(bits).view(np.float64)   # the C == on doubles
        else:
            eq = c == np.uint64(bits)
        return sum(1 << int(r) for r in np.nonzero(used & eq)[0])

    def _find(self, col, bits, want, result):
        if col < 0 or col >= self.cols or self.types[col] != want:
            return -1
        m = self.mask(col, bits)
        result.extend(r for r in range(self.rows) if (m >> r) & 1)
        return len(result)

    def find_int(self, col, value, result):
        return self._find(col, i64_bits(value), INT, result)

    def find_float(self, col, value, result):
        return self._find(col, f64_bits(value), FLOAT, result)

    def find_row_by_col_value(self, col, var, result):
        """var: a list of (type, value).  The type of var's element 0 is tested against the
        column, then the value is read at index `col` of var (RC:794): 0 / 0.0 past var's end or
        for an element of another type (NFCDataList::Int / Float)."""
        if col < 0 or col >= self.cols:
            return -1
        t0 = var[0][0] if var else None
        if t0 != self.types[col]:
            return -1
        v = var[col][1] if col < len(var) and var[col][0] == t0 else 0
        return self.find_int(col, v, result) if t0 == INT else self.find_float(col, v, result)

    def query_row(self, row):
        """the row's cells (bit patterns) or None: an invalid or unused row (the reference's false)"""
        if row < 0 or row >= self.rows or not self.is_used(row):
            return None
        return [int(self.cells[c, row]) for c in range(self.cols)]


# ---- the golden world: a script of text lines ----
#   REC <name> <rows> <types: I / F per column>       OBJ <n objects>
#   INIT <obj> <rec> <row> <values>                   a creation-time row (before the first window)
#   SI <obj> <rec> <row> <col> <int>                  SetRecordInt
#   RM <obj> <rec> <row>                              Remove
#   AR <obj> <rec> <row | -1> [<values>]              AddRow (no values: the initial 0s)
#   CL <obj> <rec>                                    ClearRecord
#   X                                                 the frame (nothing for the reference)
#   FI[+] <obj> <rec> <col> <int>                     FindInt     ("+": the list of the find before is kept)
#   FF[+] <obj> <rec> <col> <float>                   FindFloat
#   FV[+] <obj> <rec> <col> <n> <type> <value> ...    FindRowByColValue with a var of n elements
#   QR <obj> <rec> <row>                              QueryRow
# A value is an int in decimal or a float as C99 hex (float.hex()); rec = number of records: an
# unknown record name; obj = number of objects: an unknown NFGUID.  Each find / QR answers one line
#   A <k> <ret> : <list>        (QR: ret 0 / 1 and the row's cells as uint64 bit patterns)
GOLDEN_RECORDS = [("Bag", 16, "IIF"), ("Wide", 64, "IF")]
GOLDEN_OBJECTS = 24
FLOATS = [0.0, 0.5, 1.5, -2.25]


def _val(t, v):
    return str(int(v)) if t == "I" else float(v).hex()


def golden_script():
    rnd = random.Random(20261020)
    L = [f"REC {n} {r} {t}" for n, r, t in GOLDEN_RECORDS] + [f"OBJ {GOLDEN_OBJECTS}"]
    rows_of = [r for _, r, _ in GOLDEN_RECORDS]
    types_of = [t for _, _, t in GOLDEN_RECORDS]

    def values(rec):
        return " ".join(_val(t, rnd.randrange(0, 4) if t == "I" else rnd.choice(FLOATS)) for t in types_of[rec])

    for o in range(GOLDEN_OBJECTS):
        for r in sorted(rnd.sample(range(16), rnd.randrange(0, 9))):
            L.append(f"INIT {o} 0 {r} {values(0)}")
        wide = sorted(rnd.sample(range(64), rnd.randrange(0, 6)))
        if o % 5 == 0 and 63 not in wide:
            wide.append(63)
        for r in wide:
            L.append(f"INIT {o} 1 {r} {values(1)}")
    L.append("INIT 1 1 63 3 0x1.8p+0")   # the find that hits row 63 (window 0, after the frame)

    def finds(objs):
        for o in objs:
            rec = rnd.randrange(2)
            L.append(f"FI {o} {rec} {rnd.randrange(2) if rec == 0 else 0} {rnd.randrange(0, 4)}")
            L.append(f"FF {o} {rec} {2 if rec == 0 else 1} {rnd.choice(FLOATS).hex()}")
        o = objs[0]
        L.append(f"QR {o} 0 {rnd.randrange(16)}")
        L.append(f"QR {o} 1 63")

    for t in range(4):
        touched = rnd.sample(range(GOLDEN_OBJECTS), 8)
        for o in touched[:6]:
            L.append(f"SI {o} 0 {rnd.randrange(16)} {rnd.randrange(2)} {rnd.randrange(0, 4)}")
            L.append(f"RM {o} {rnd.randrange(2)} {rnd.randrange(16)}")
            L.append(f"AR {o} 0 -1")
            r = rnd.randrange(16)
            L.append(f"AR {o} 0 {r} {values(0)}")
            L.append(f"AR {o} 1 {rnd.choice([63, rnd.randrange(64)])} {values(1)}")
        L.append(f"CL {touched[6]} 0")
        L.append(f"CL {touched[7]} 1")
        L.append(f"AR {touched[7]} 1 -1")
        # a removed row's stale cell, then the row re-added without values: it holds 0
        o = touched[0]
        L += [f"AR {o} 0 5 3 3 0x1.8p+0", f"RM {o} 0 5", f"FI {o} 0 0 3", f"AR {o} 0 5", f"FI {o} 0 0 0",
              f"FI {o} 0 0 3", f"FF {o} 0 2 0x0p+0", f"QR {o} 0 5"]
        others = [o for o in range(GOLDEN_OBJECTS) if o not in touched]
        finds(touched[:4] + rnd.sample(others, 4))               # mid-window: host and device answers
        # the list is appended to and the return value is its total size
        L += [f"FI {touched[1]} 0 0 1", f"FI+ {touched[1]} 0 1 2", f"FF+ {others[0]} 0 2 0x1p-1"]
        # FindRowByColValue: var's element 0 gives the type, element nCol the value
        L += [f"FV {others[1]} 0 0 1 I 2", f"FV {others[1]} 0 1 1 I 2", f"FV {others[1]} 0 1 2 I 2 I 1",
              f"FV {others[1]} 0 1 2 I 2 F 0x1p+0", f"FV {others[1]} 0 2 3 F 0x1.8p+0 I 1 F 0x1p-1",
              f"FV {others[1]} 0 2 1 F 0x1.8p+0", f"FV {others[1]} 0 2 1 I 1", f"FV {others[1]} 0 0 0",
              f"FV {touched[2]} 1 1 2 F 0x1p-1 F 0x1.8p+0"]
        # -1: a column of another type, a column outside the record, an unknown record, an unknown object
        L += [f"FI {others[2]} 0 2 0", f"FF {others[2]} 0 0 0x0p+0", f"FI {others[2]} 0 3 1", f"FI {others[2]} 0 -1 1",
              f"FI {others[2]} 2 0 1", f"FI {GOLDEN_OBJECTS} 0 0 1", f"FI+ {others[2]} 1 1 0"]
        L.append("X")
        finds(touched[:4] + rnd.sample(others, 4))               # after the frame applied the calls
        L += [f"FI {touched[0]} 0 0 0", f"QR {touched[0]} 0 5", f"FI {touched[7]} 1 0 0", f"FF {touched[7]} 1 1 0x0p+0"]
        if t == 0:
            L += ["FI 1 1 0 3", "FF 1 1 1 0x1.8p+0", "QR 1 1 63"]
    return L


def _parse_values(tok, types):
    return [i64_bits(int(v)) if t == "I" else f64_bits(float.fromhex(v)) for t, v in zip(types, tok)]


def replay(script):
    """the script's answers by the model: [[ret, list]] per find / QR line, in order"""
    recs, types, objs, out, last = [], [], [], [], []
    for ln in script:
        f = ln.split()
        op = f[0]
        if op == "REC":
            recs.append((int(f[2]), [FLOAT if c == "F" else INT for c in f[3]]))
            types.append(f[3])
            continue
        if op == "OBJ":
            objs = [[Record(r, t) for r, t in recs] for _ in range(int(f[1]))]
            continue
        if op == "X":
            continue
        o, r = int(f[1]), int(f[2])
        known = 0 <= o < len(objs) and 0 <= r < len(recs)
        rec = objs[o][r] if known else None
        if op in ("INIT", "AR"):
            rec.add_row(int(f[3]), _parse_values(f[4:], types[r]) if len(f) > 4 else None)
        elif op == "SI":
            rec.set_int(int(f[3]), int(f[4]), int(f[5]))
        elif op == "RM":
            rec.remove(int(f[3]))
        elif op == "CL":
            rec.clear()
        elif op == "QR":
            q = rec.query_row(int(f[3])) if known else None
            out.append([0 if q is None else 1, q or []])
        else:
            if not op.endswith("+"):
                last = []
            col = int(f[3])
            if not known:
                ret = -1
            elif op[:2] == "FI":
                ret = rec.find_int(col, int(f[4]), last)
            elif op[:2] == "FF":
                ret = rec.find_float(col, float.fromhex(f[4]), last)
            else:
                var = [(INT, int(f[6 + 2 * k])) if f[5 + 2 * k] == "I" else (FLOAT, float.fromhex(f[6 + 2 * k]))
                       for k in range(int(f[4]))]
                ret = rec.find_row_by_col_value(col, var, last)
            out.append([ret, list(last)])
    return out
