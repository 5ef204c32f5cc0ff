"""The reference's NFCRecord::SwapRowInfo (RC:1219-1253) restated over tests/record_object_model.ORecord
(test infrastructure).

SRecord adds swap_row_info(origin, target) to ORecord's calls: refused (false, nothing changes) on an
origin that is not a used row — an origin outside the record counts as not used — and on a target
outside the record; else every cell of the two rows and the two used states change places and ONE
event is logged, (EV_SWAP, origin, target, NULL_OBJECT, NULL_OBJECT): the hook's nRow is the origin,
its nCol the target ROW.  origin == target on a used row logs the event and changes nothing.  No
Update is logged for a moved cell.

coalesce() is record_object_model.coalesce with the one rule a Swap adds: the per-cell log follows the
row.  Per record the row events first, in call order, Swap among them; then one Update per cell in
(row, col) order from the first logged old value to the last logged new one, dropped when all bits
are equal — where the (row, col) key of every log entry made before a Swap of rows a, b is re-keyed
a <-> b by that Swap.  A client that applies the events in order ends in the server's state
(apply_events()).

golden_script() is the world of tests/golden/record_swap.json: record_object_model's line format plus
    SW <obj> <rec> <origin> <target>          SwapRowInfo
replayed by tests/cpp/record_swap_ref.cpp (the compiled reference) and by replay() here.
"""
import random

import numpy as np

from tests import record_object_model as rom
from tests.record_object_model import (EV_ADD, EV_COVER, EV_DEL, EV_UPDATE, NULL_OBJECT, ORecord, flat_event, flat_row,
                                       parse_guid, parse_values, u64)

EV_SWAP = 4


class SRecord(ORecord):
    def swap_row_info(self, origin, target):
        if origin < 0 or origin >= self.rows or not self.is_used(origin):   # RC:1221 (IsUsed of a row outside: false)
            return False
        if target < 0 or target >= self.rows:                               # RC:1226 ValidRow
            return False
        if origin != target:
            a, b = self.cells[:, origin].copy(), self.cells[:, target].copy()
            self.cells[:, origin], self.cells[:, target] = b, a
            ub = (self.used >> target) & 1                                   # (the origin's bit is set)
            self.used = (self.used & ~(1 << origin)) | (ub << origin) | (1 << target)
        self.events.append((EV_SWAP, origin, target, NULL_OBJECT, NULL_OBJECT))
        return True


def coalesce(events):
    """one record's hook events of a window -> the frame's record events of it"""
    rows = [e for e in events if e[0] != EV_UPDATE]
    first, last = {}, {}
    for op, row, col, old, new in events:
        if op == EV_UPDATE:
            first.setdefault((row, col), old)
            last[(row, col)] = new
        elif op == EV_SWAP and row != col:       # the logs of rows `row` and `col` change places
            other = {row: col, col: row}
            for d in (first, last):
                moved = {(other[r], c): d.pop((r, c)) for r, c in list(d) if r in other}
                d.update(moved)
    cells = [(EV_UPDATE, row, col, first[(row, col)], last[(row, col)]) for row, col in sorted(first)
             if first[(row, col)] != last[(row, col)]]
    return rows + cells


def apply_events(rec, events, final):
    """A client's copy `rec` (an SRecord in the pre-window state) taken through the frame's events in
    order: Swap as a row exchange, Del clears the used bit, Add / Cover set it and the row takes the
    values it ends the window with (the events carry none: the client reads them; such a row's Updates
    are already in those values).  Asserts that every Update of a row no Add / Cover wrote finds its old
    value in the copy.  `final`: the server's record after the window."""
    fresh = [False] * rec.rows       # the row's cells come from `final` (travels with the row)
    for op, row, col, old, new in events:
        if op == EV_SWAP:
            if row != col:
                a, b = rec.cells[:, row].copy(), rec.cells[:, col].copy()
                rec.cells[:, row], rec.cells[:, col] = b, a
                ua, ub = (rec.used >> row) & 1, (rec.used >> col) & 1
                rec.used = (rec.used & ~((1 << row) | (1 << col))) | (ub << row) | (ua << col)
                fresh[row], fresh[col] = fresh[col], fresh[row]
        elif op in (EV_ADD, EV_COVER):
            rec.used |= 1 << row
            fresh[row] = True
        elif op == EV_DEL:
            rec.used &= ~(1 << row)
        elif not fresh[row]:
            assert rec._value(row, col) == old, ("an Update's old value is not what the client holds", row, col)
            p = rec.phys[col]
            if rec.logical[col] == "O":
                rec.cells[p, row], rec.cells[p + 1, row] = u64(new[1]), u64(new[0])
            else:
                rec.cells[p, row] = u64(new[1])
    for row in range(rec.rows):
        if fresh[row]:
            rec.cells[:, row] = final.cells[:, row]
    return rec


# ---- the golden world ----
GOLDEN_RECORDS = [("Hero", 16, "OIF"), ("Team", 64, "O"), ("Pair", 5, "OO"), ("Edge", 20, "I" * 14 + "O"), ("One", 1, "I")]
GOLDEN_OBJECTS = 24
GOLDEN_WINDOWS = 3
GOLDEN_SEED = 20261107   # (chosen so that check_conditions holds)
GUIDS = rom.GUIDS
FLOATS = rom.FLOATS


def golden_script(seed=GOLDEN_SEED):
    """The generator keeps the model beside the script, so that a line meant as a move, a refusal or
    a chain is one when it is replayed; check_conditions() counts them again from the answers."""
    rnd = random.Random(seed)
    L = [f"REC {n} {r} {t}" for n, r, t in GOLDEN_RECORDS] + [f"OBJ {GOLDEN_OBJECTS}"]
    rows_of = [r for _, r, _ in GOLDEN_RECORDS]
    types_of = [t for _, _, t in GOLDEN_RECORDS]
    nrec = len(GOLDEN_RECORDS)
    objs = [[SRecord(r, t) for _, r, t in GOLDEN_RECORDS] for _ in range(GOLDEN_OBJECTS)]

    def values(rec):
        return " ".join(rom._val(t, rnd.choice(GUIDS) if t == "O" else rnd.randrange(0, 4) if t == "I" else rnd.choice(FLOATS))
                        for t in types_of[rec])

    def emit(ln):
        L.append(ln)
        f = ln.split()
        if f[0] in ("X", "QR", "GO", "FO", "FI"):
            return
        o, r = int(f[1]), int(f[2])
        if not (0 <= o < GOLDEN_OBJECTS and 0 <= r < nrec):
            return
        rec = objs[o][r]
        if f[0] in ("INIT", "AR"):
            rec.add_row(int(f[3]), parse_values(f[4:], rec.logical) if len(f) > 4 else None)
        elif f[0] == "SO":
            rec.set_object(int(f[3]), int(f[4]), parse_guid(f[5]))
        elif f[0] == "SI":
            rec.set_int(int(f[3]), int(f[4]), int(f[5]))
        elif f[0] == "RM":
            rec.remove(int(f[3]))
        elif f[0] == "CL":
            rec.clear()
        elif f[0] == "SW":
            rec.swap_row_info(int(f[3]), int(f[4]))

    for o in range(GOLDEN_OBJECTS):
        for rec in range(nrec):
            k = rnd.randrange(2, min(rows_of[rec], 8) + 1) if rows_of[rec] > 1 else o % 2
            rows = sorted(rnd.sample(range(rows_of[rec]), k))
            if rec == 1 and o % 3 == 0 and 63 not in rows:
                rows.append(63)
            for r in rows:
                emit(f"INIT {o} {rec} {r} {values(rec)}")

    def used(o, r):
        return [x for x in range(rows_of[r]) if objs[o][r].is_used(x)]

    def free(o, r):
        return [x for x in range(rows_of[r]) if not objs[o][r].is_used(x)]

    def a_set(o, r, row):
        """a Set on (o, r, row) that changes the cell"""
        t = types_of[r]
        if "I" in t and rnd.random() < 0.5:
            c = t.index("I")
            cur = int(objs[o][r].cells[objs[o][r].phys[c], row])
            emit(f"SI {o} {r} {row} {c} {(cur + 1 + rnd.randrange(3)) % 5}")
        elif "O" in t:
            c = rnd.choice([i for i, x in enumerate(t) if x == "O"])
            cur = objs[o][r]._value(row, c)
            emit(f"SO {o} {r} {row} {c} {rom._val('O', rnd.choice([g for g in GUIDS if g != cur]))}")
        else:
            cur = int(objs[o][r].cells[0, row])
            emit(f"SI {o} {r} {row} 0 {(cur + 1) % 5}")

    def reads(o, r):
        t = types_of[r]
        emit(f"QR {o} {r} {rnd.randrange(rows_of[r])}")
        if "O" in t:
            c = t.index("O")
            emit(f"FO {o} {r} {c} {rom._val('O', rnd.choice(GUIDS))}")
            emit(f"GO {o} {r} {rnd.randrange(rows_of[r])} {c}")
        if "I" in t:
            emit(f"FI {o} {r} {t.index('I')} {rnd.randrange(0, 4)}")

    for w in range(GOLDEN_WINDOWS):
        touched = rnd.sample(range(GOLDEN_OBJECTS), 8)
        for o in touched:
            for r in rnd.sample(range(4), 3) + [4]:
                u, fr = used(o, r), free(o, r)
                if r == 4:                                   # the one-row record
                    emit(f"SW {o} 4 0 0")
                    emit(f"SW {o} 4 0 1")
                    if w % 2 == 0:
                        emit(f"SI {o} 4 0 0 {rnd.randrange(5)}")
                        emit(f"SW {o} 4 0 0")
                    continue
                if len(u) < 3:                               # rows to work with
                    for _ in range(3):
                        emit(f"AR {o} {r} -1 {values(r)}")
                    u, fr = used(o, r), free(o, r)
                top = rows_of[r] - 1
                a, b = rnd.sample(u, 2)
                emit(f"SW {o} {r} {a} {b}")                  # used <-> used
                if r == 1 and rnd.random() < 0.7:            # row 63 of Team: as origin or as target
                    if objs[o][r].is_used(63):
                        emit(f"SW {o} {r} 63 {rnd.randrange(63)}")
                    else:
                        emit(f"SW {o} {r} {rnd.choice(used(o, r))} 63")
                if fr:
                    u, fr = used(o, r), free(o, r)
                    a = rnd.choice(u)
                    a_set(o, r, a)                           # a Set, then a Swap of its row: a move
                    emit(f"SW {o} {r} {a} {rnd.choice(fr)}")
                u, fr = used(o, r), free(o, r)
                if fr:
                    emit(f"SW {o} {r} {rnd.choice(fr)} {rnd.choice(u)}")        # origin unused: refused
                emit(f"SW {o} {r} {rnd.choice([-1, rows_of[r], rows_of[r] + 5])} {rnd.choice(u)}")
                emit(f"SW {o} {r} {rnd.choice(u)} {rnd.choice([-1, rows_of[r], 200])}")
                a = rnd.choice(u)
                emit(f"SW {o} {r} {a} {a}")                  # origin == target
                if fr:                                       # a Swap, then a Set on the moved row
                    a, b = rnd.choice(u), rnd.choice(fr)
                    emit(f"SW {o} {r} {a} {b}")
                    a_set(o, r, b)
                u = used(o, r)
                if len(u) >= 3:                              # a chain a <-> b, b <-> c behind a Set of a
                    a, b, c = rnd.sample(u, 3)
                    a_set(o, r, a)
                    emit(f"SW {o} {r} {a} {b}")
                    emit(f"SW {o} {r} {b} {c}")
                u, fr = used(o, r), free(o, r)
                low = [x for x in u if fr and x < fr[0]]
                if low:                                      # a move frees a row below every unused one
                    a = rnd.choice(low)
                    emit(f"SW {o} {r} {a} {rnd.choice(fr)}")
                    emit(f"AR {o} {r} -1" + (f" {values(r)}" if rnd.random() < 0.5 else ""))
                if rnd.random() < 0.3:
                    emit(f"RM {o} {r} {rnd.choice(used(o, r))}")
                if rnd.random() < 0.3:
                    emit(f"AR {o} {r} {rnd.randrange(rows_of[r])} {values(r)}")
                if rnd.random() < 0.08:
                    emit(f"CL {o} {r}")
                if rnd.random() < 0.4:
                    emit(f"SW {o} {r} {top} 0")              # the last row <-> row 0, whatever their state
                if rnd.random() < 0.5:
                    reads(o, r)                              # mid-window
        # an unknown record / object
        emit(f"SW {touched[0]} {nrec} 0 1")
        emit(f"SW {GOLDEN_OBJECTS} 0 0 1")
        emit("X")
        for o in touched[:3]:
            for r in range(4):
                reads(o, r)                                  # after the frame applied the calls
            emit(f"QR {o} 4 0")
            emit(f"QR {o} 1 63")
    return L


def replay(script, on_call=None):
    """record_object_model.replay with the SW line: [ret, list, events] per call line, in order"""
    defs, objs, out, last = [], [], [], []
    for ln in script:
        f = ln.split()
        op = f[0]
        if op == "REC":
            defs.append((int(f[2]), f[3]))
            continue
        if op == "OBJ":
            objs = [[SRecord(r, t) for r, t in defs] for _ in range(int(f[1]))]
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
        elif op == "SW":
            ret = int(known and rec.swap_row_info(int(f[3]), int(f[4])))
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
            else:
                ret = rec.find_int(col, int(f[4]), last)
            lst = list(last)
        ev = [flat_event(e) for e in rec.events[n0:]] if known else []
        out.append([int(ret), lst, ev])
    return out


CONDITIONS = ("used<->used", "move", "origin unused", "origin out of range", "target out of range", "origin == target",
              "swap after a set of its row", "set after a swap on the moved row", "chain", "AddRow(-1) takes the freed row",
              "row 63 of Team", "rows of Edge")


def count_conditions(script, answers):
    """how often each of CONDITIONS occurs in the script, from the answers and the replayed state"""
    n = dict.fromkeys(CONDITIONS, 0)
    st = {"prev": None, "sets": {}, "moved": {}, "swaps": {}}

    def watch(k, ln, f, objs):
        if k is None:                       # the frame: the windows' memories end
            st["sets"], st["moved"], st["swaps"], st["prev"] = {}, {}, {}, None
            return
        op = f[0]
        o, r = int(f[1]), int(f[2])
        known = 0 <= o < len(objs) and 0 <= r < len(objs[o])
        key = (o, r)
        prev, st["prev"] = st["prev"], None
        if not known:
            return
        rec = objs[o][r]
        ok = answers[k][0] == 1
        if op in ("SI", "SO") and ok:
            row = int(f[3])
            st["sets"].setdefault(key, set()).add(row)
            if row in st["moved"].get(key, ()):
                n["set after a swap on the moved row"] += 1
        elif op == "SW":
            a, b = int(f[3]), int(f[4])
            inr = lambda x: 0 <= x < rec.rows
            if not ok:
                if not inr(a):
                    n["origin out of range"] += 1
                elif not rec.is_used(a):
                    n["origin unused"] += 1
                elif not inr(b):
                    n["target out of range"] += 1
                return
            if a == b:
                n["origin == target"] += 1
                return
            move = not rec.is_used(b)
            n["move" if move else "used<->used"] += 1
            if a in st["sets"].get(key, ()) or b in st["sets"].get(key, ()):
                n["swap after a set of its row"] += 1
            if any(a in p or b in p for p in st["swaps"].get(key, [])):
                n["chain"] += 1
            st["swaps"].setdefault(key, []).append((a, b))
            st["moved"].setdefault(key, set()).update((a, b))
            # the Sets' rows travel with the swap
            s = st["sets"].get(key)
            if s:
                st["sets"][key] = {b if x == a else a if x == b else x for x in s}
            if r == 1 and 63 in (a, b):
                n["row 63 of Team"] += 1
            if r == 3:
                n["rows of Edge"] += 1
            if move and all(x > a for x in range(rec.rows) if not rec.is_used(x)):
                st["prev"] = (key, a)
        elif op == "AR" and int(f[3]) == -1 and prev and prev[0] == key and answers[k][0] == prev[1]:
            n["AddRow(-1) takes the freed row"] += 1
    got = replay(script, watch)
    assert got == answers, "the model does not replay the answers"
    return n


def check_conditions(script, answers):
    """what the golden is there for: each condition at least 20 times (the generator asserts it,
    tests/test_record_swap.py again)"""
    n = count_conditions(script, answers)
    for name in CONDITIONS:
        assert n[name] >= 20, (name, n[name])
    return n


def random_window(rng, rec, n_calls):
    """n_calls random calls on `rec` (an SRecord), Swaps among Sets and row calls; values from the
    golden's small domains so that Sets meet equal values too"""
    lg, rows = rec.logical, rec.rows
    for _ in range(n_calls):
        k = int(rng.integers(0, 12))
        # (mostly a few low rows and the last one, so that Sets and Swaps meet on a row)
        near = lambda: int(rng.choice([0, 1, 2, 3, rows - 1])) % rows if rng.random() < 0.7 else int(rng.integers(0, rows))
        row = near()
        if k < 4:
            rec.swap_row_info(row, near())
        elif k < 7:
            c = int(rng.integers(0, len(lg)))
            if lg[c] == "O":
                rec.set_object(row, c, GUIDS[int(rng.integers(0, len(GUIDS)))])
            elif lg[c] == "I":
                rec.set_int(row, c, int(rng.integers(0, 4)))
        elif k < 8:
            rec.remove(row)
        elif k < 9:
            rec.add_row(-1)
        elif k < 11:
            rec.add_row(row, [GUIDS[int(rng.integers(0, len(GUIDS)))] if t == "O" else
                              rom.f64_bits(FLOATS[int(rng.integers(0, 3))]) if t == "F" else int(rng.integers(0, 4))
                              for t in lg])
        elif int(rng.integers(0, 4)) == 0:
            rec.clear()


def clone(rec):
    c = SRecord(rec.rows, rec.logical)
    c.cells = rec.cells.copy()
    c.used = rec.used
    return c

