"""The reference's enter snapshots restated in Python (test infrastructure).

What NFCGameServerNet_ServerModule::OnPropertyEnter (:271-393) and OnRecordEnter (:395-554) pack for
an object and a view.  The private view (the recipient is the object itself) holds the entries whose
flags have PRIVATE, the public view those with PUBLIC.  The property walk is NFCPropertyManager's
First / Next over a std::map keyed by name: BYTE-WISE NAME ORDER; a property is packed when
NFCProperty::Changed() holds, i.e. !IsNullValue() (NFIDataList.h:160-221): an int != 0, an f64 v with
v > 0.001 || v < -0.001 (so 0.001, -0.001, -0.0, denormals and NaN are not packed), an object whose
NFGUID has a non-zero half.  The record walk is in name order too; every record in view is one entry,
also without a used row, holding its used rows ascending and every column of each (no null test on
cells; an unused row's cell is never packed).

Values are uint64 bit patterns.  golden_script() is the world of tests/golden/enter_snapshot.json:
text lines that tests/cpp/enter_snapshot_ref.cpp (the compiled reference) and
tests/cpp/enter_snapshot_plugin.cpp (the C++ plugin on a GPU) both replay, and replay() here.
"""
import random

import numpy as np

from tests.record_find_model import FLOAT, INT, Record, f64_bits, i64_bits

OBJECT = 2
PUBLIC, PRIVATE, UPLOAD = 1, 2, 4


def name_order(names):
    """indices of names in the order of std::map<std::string, ...>: byte-wise"""
    return sorted(range(len(names)), key=lambda i: names[i].encode())


def is_set(ptype, bits, head=0):
    """NFCProperty::Changed(): !IsNullValue()"""
    if ptype == INT:
        return int(bits) != 0
    if ptype == FLOAT:
        v = float(np.uint64(bits).view(np.float64))
        return v > 0.001 or v < -0.001   # (the two ordered compares: a NaN is null)
    return int(bits) != 0 or int(head) != 0


class Obj:
    """One object: named properties (name, type, flags) with their values, named records
    (name, flags, Record)."""

    def __init__(self, props, recs):
        self.props = [(n, int(t), int(f)) for n, t, f in props]
        self.recs = list(recs)
        self.val = {n: (0, 0) for n, _, _ in self.props}   # (bits / data half, head half)

    def load(self, name, bits, head=0):
        """a value put in place as it is (creation time)"""
        self.val[name] = (int(bits), int(head))

    def set(self, name, bits, head=0):
        """SetPropertyInt / Float / Object (PR:254-334, PR:395): a float within 1e-15 of the held
        value is not taken (IsZeroDouble)"""
        t = next(t for n, t, _ in self.props if n == name)
        if t == FLOAT:
            new = float(np.uint64(bits).view(np.float64))
            cur = float(np.uint64(self.val[name][0]).view(np.float64))
            if abs(new - cur) <= 1e-15:
                return
        self.val[name] = (int(bits), int(head))


def view(obj, private):
    """([(name, bits) | (name, bits, head)], [(record name, used mask, row-major cells)])"""
    flag = PRIVATE if private else PUBLIC
    pl = []
    for i in name_order([p[0] for p in obj.props]):
        n, t, f = obj.props[i]
        b, h = obj.val[n]
        if (f & flag) and is_set(t, b, h):
            pl.append((n, b, h) if t == OBJECT else (n, b))
    rl = []
    for i in name_order([r[0] for r in obj.recs]):
        n, f, rec = obj.recs[i]
        if not (f & flag):
            continue
        cells = [int(rec.cells[c, r]) for r in range(rec.rows) if rec.is_used(r) for c in range(rec.cols)]
        rl.append((n, rec.used, cells))
    return pl, rl


# ---- the golden world: a script of text lines ----
#   PROP <name> <I | F | O> <flags>                   REC <name> <rows> <types> <flags>
#   OBJ <n objects>                                   (every object has every property and record)
#   SI <obj> <prop> <int>        SF <obj> <prop> <float as C99 hex>       SO <obj> <prop> <head> <data>
#   AR <obj> <rec> <row | -1> [<values>]              AddRow (no values: the initial 0s)
#   RI <obj> <rec> <row> <col> <int>                  SetRecordInt
#   RM <obj> <rec> <row>         CL <obj> <rec>       Remove / Clear
#   X                                                 the frame (nothing for the reference)
#   S <obj> <0 public | 1 private>                    one snapshot; it answers the lines
#       V <k> <n props> <n records>
#       P <name> <bits> [<head>]                      (an object property: data half, head half)
#       R <name> <used mask> : <cells, used rows ascending x columns>
GOLDEN_PROPS = [
    ("Zeta", "I", PUBLIC), ("alpha", "I", PUBLIC | PRIVATE), ("a9", "F", PUBLIC), ("a10", "F", PRIVATE | PUBLIC),
    ("Beta", "O", PUBLIC), ("hidden", "I", 0), ("up", "I", UPLOAD), ("mine", "F", PRIVATE), ("b", "I", PRIVATE),
    ("Owner", "O", PRIVATE), ("B", "F", PUBLIC | UPLOAD), ("m", "I", PUBLIC),
]
GOLDEN_RECORDS = [("bag", 8, "IIF", PUBLIC), ("Wide", 64, "IF", PRIVATE), ("Empty", 4, "I", PUBLIC | PRIVATE),
                  ("none", 4, "I", 0), ("Both", 5, "FI", PUBLIC | PRIVATE)]
GOLDEN_OBJECTS = 12
# the null test's boundary values: kept (the doubles next to +-0.001 on the far side, ordinary values)
# and dropped (0.001, -0.001, -0.0, a denormal, NaN)
F_KEPT = [float(np.nextafter(0.001, 1.0)), float(np.nextafter(-0.001, -1.0)), 1.5, -2.25, 1e300]
F_DROPPED = [0.001, -0.001, -0.0, 5e-324, float("nan"), 0.0005]
I_VALUES = [1, -1, 1 << 32, -(1 << 63), 7, 0]


def _val(t, v):
    return str(int(v)) if t == "I" else float(v).hex()


def golden_script():
    rnd = random.Random(20261021)
    L = [f"PROP {n} {t} {f}" for n, t, f in GOLDEN_PROPS]
    L += [f"REC {n} {r} {t} {f}" for n, r, t, f in GOLDEN_RECORDS] + [f"OBJ {GOLDEN_OBJECTS}"]
    ints = [n for n, t, _ in GOLDEN_PROPS if t == "I"]
    flts = [n for n, t, _ in GOLDEN_PROPS if t == "F"]
    objs = [n for n, t, _ in GOLDEN_PROPS if t == "O"]

    def snaps(which):
        for o in which:
            L.append(f"S {o} 0")
            L.append(f"S {o} 1")

    # window 0: object 0 untouched (empty views but the records in view); the boundary values one
    # object each; a removed row that keeps its value; a record in view that never has a row
    for k, v in enumerate(F_KEPT + F_DROPPED):
        o = 1 + k % (GOLDEN_OBJECTS - 1)
        for n in flts:
            L.append(f"SF {o} {n} {float(v).hex()}")
    for k, v in enumerate(I_VALUES):
        o = 1 + k
        for n in ints:
            L.append(f"SI {o} {n} {v}")
    L += ["SO 1 Beta 0 5", "SO 1 Owner 9 0", "SO 2 Beta 3 4", "SO 2 Owner 0 0", "SO 3 Beta 1 1", "SO 3 Beta 0 0"]
    L += ["AR 1 bag 2 11 0 0x1.8p+0", "AR 1 bag 0 -3 4294967296 -0x0p+0", "RM 1 bag 2",
          "AR 2 bag -1", "AR 2 bag -1 5 6 0x1p-1", "RI 2 bag 0 1 77", "RI 2 bag 5 1 78",
          "AR 3 Wide 63 9 0x1p+0", "AR 3 Wide 0", "AR 3 Both 4 nan 0", "AR 4 Both 1 0x1p-1074 -9", "CL 4 Both",
          "AR 5 Wide 10 1 0x1p+1", "RM 5 Wide 10", "AR 5 Wide 11 2 0x1p+2"]
    snaps(range(GOLDEN_OBJECTS))
    L.append("X")
    snaps(range(6))
    # windows 1..2: random Sets (to 0 and back among them) and row calls, snapshots mid-window and
    # after the frame
    for w in range(2):
        for _ in range(40):
            o = rnd.randrange(GOLDEN_OBJECTS)
            k = rnd.randrange(10)
            if k < 3:
                L.append(f"SI {o} {rnd.choice(ints)} {rnd.choice(I_VALUES)}")
            elif k < 5:
                L.append(f"SF {o} {rnd.choice(flts)} {float(rnd.choice(F_KEPT + F_DROPPED)).hex()}")
            elif k < 6:
                L.append(f"SO {o} {rnd.choice(objs)} {rnd.choice([0, 0, 7])} {rnd.choice([0, 3])}")
            else:
                n, rows, types, _ = rnd.choice(GOLDEN_RECORDS[:2] + GOLDEN_RECORDS[4:])
                j = rnd.randrange(5)
                if j < 2:
                    vals = " ".join(_val(t, rnd.choice(I_VALUES) if t == "I" else rnd.choice(F_KEPT + [0.0])) for t in types)
                    L.append(f"AR {o} {n} {rnd.choice([-1, rnd.randrange(rows)])} {vals}")
                elif j < 3:
                    L.append(f"AR {o} {n} -1")
                elif j < 4:
                    L.append(f"RM {o} {n} {rnd.randrange(min(rows, 8))}")
                else:
                    c = types.index("I")
                    L.append(f"RI {o} {n} {rnd.randrange(min(rows, 8))} {c} {rnd.choice(I_VALUES)}")
        snaps(range(GOLDEN_OBJECTS))
        L.append("X")
        snaps(range(0, GOLDEN_OBJECTS, 2))
    return L


def _bits(t, tok):
    if t == "I":
        return i64_bits(int(tok))
    return f64_bits(float("nan") if tok == "nan" else float.fromhex(tok))


def replay(script):
    """the model's answers: one [[(name, bits[, head])], [(rec, used, cells)]] per S line"""
    props, recs, objs, out = [], [], [], []
    tcode = {"I": INT, "F": FLOAT, "O": OBJECT}
    for ln in script:
        f = ln.split()
        op = f[0]
        if op == "PROP":
            props.append((f[1], tcode[f[2]], int(f[3])))
        elif op == "REC":
            recs.append((f[1], int(f[2]), f[3], int(f[4])))
        elif op == "OBJ":
            for _ in range(int(f[1])):
                objs.append(Obj(props, [(n, fl, Record(rows, [tcode[c] for c in ty])) for n, rows, ty, fl in recs]))
        elif op == "X":
            continue
        elif op == "S":
            pl, rl = view(objs[int(f[1])], f[2] == "1")
            out.append([[list(p) for p in pl], [[n, u, c] for n, u, c in rl]])
        elif op in ("SI", "SF", "SO"):
            o = objs[int(f[1])]
            if op == "SO":
                o.set(f[2], i64_bits(int(f[4])), i64_bits(int(f[3])))
            else:
                o.set(f[2], _bits("I" if op == "SI" else "F", f[3]))
        else:
            o = objs[int(f[1])]
            ri = next(i for i, r in enumerate(recs) if r[0] == f[2])
            rec, types = o.recs[ri][2], recs[ri][2]
            if op == "AR":
                vals = [_bits(t, x) for t, x in zip(types, f[4:])] if len(f) > 4 else None
                rec.add_row(int(f[3]), vals)
            elif op == "RI":
                rec.set_int(int(f[3]), int(f[4]), int(f[5]))
            elif op == "RM":
                rec.remove(int(f[3]))
            elif op == "CL":
                rec.clear()
    return out
