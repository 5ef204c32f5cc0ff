"""CPU: the enter-snapshot entry points exist and refuse a null world; the model
(tests/enter_snapshot_model.py) on a hand-sized object; the model equals every answer the compiled
reference recorded (tests/golden/enter_snapshot.json)."""
import ctypes
import json
import os

import numpy as np

from noahgameframe_amd import kernel
from tests import enter_snapshot_model as esm
from tests.enter_snapshot_model import FLOAT, INT, OBJECT, PRIVATE, PUBLIC, UPLOAD, Obj, Record, f64_bits, i64_bits, view
from tests.golden import gen_enter_snapshot_golden as gen

HERE = os.path.dirname(os.path.abspath(__file__))


def test_entry_points_refuse_a_null_world():
    lib = kernel.load_library()
    res = kernel.Snapshot()
    for call in (lambda: lib.nfk_snapshot_objects(None, 0, None, None, None, ctypes.byref(res)),
                 lambda: lib.nfk_snapshot_objects_obj(None, 0, None, None, ctypes.byref(res)),
                 lambda: lib.nfk_set_snapshot_order(None, None, None)):
        assert call() == -1
        assert "null" in lib.nfk_last_error().decode()


def test_model_by_hand():
    props = [("b", INT, PUBLIC), ("a9", FLOAT, PUBLIC | PRIVATE), ("a10", FLOAT, PRIVATE), ("Z", OBJECT, PUBLIC),
             ("up", INT, UPLOAD), ("none", INT, 0)]
    bag = Record(4, [INT, FLOAT])
    o = Obj(props, [("r", PUBLIC, bag), ("Q", PUBLIC | PRIVATE, Record(2, [INT])), ("p", PRIVATE, Record(2, [INT]))])
    assert view(o, False) == ([], [("Q", 0, []), ("r", 0, [])])         # nothing set: the records in view only
    assert view(o, True) == ([], [("Q", 0, []), ("p", 0, [])])
    o.set("b", 5)
    o.set("up", 5)
    o.set("none", 5)
    o.set("a9", f64_bits(0.001))
    o.set("a10", f64_bits(np.nextafter(0.001, 1)))
    o.set("Z", 0, 9)                                                   # the head half only
    assert view(o, False) == ([("Z", 0, 9), ("b", 5)], [("Q", 0, []), ("r", 0, [])])   # "Z" < "b": byte order
    assert view(o, True) == ([("a10", f64_bits(np.nextafter(0.001, 1)))], [("Q", 0, []), ("p", 0, [])])
    o.set("a9", f64_bits(-1.0))
    assert [p[0] for p in view(o, True)[0]] == ["a10", "a9"]           # "a10" < "a9"
    for v in (float("nan"), -0.0, 5e-324, -0.001):
        o.load("a9", f64_bits(v))
        assert [p[0] for p in view(o, True)[0]] == ["a10"], v
    o.set("b", 0)
    o.set("Z", 0, 0)
    assert view(o, False)[0] == []
    bag.add_row(2, [7, f64_bits(0.0)])
    bag.add_row(0, [i64_bits(-1), f64_bits(2.5)])
    bag.add_row(3, [8, 0])
    bag.remove(3)                                                      # its cells stay, and are not sent
    assert view(o, False)[1][1] == ("r", 0b101, [i64_bits(-1), f64_bits(2.5), 7, 0])


def test_model_equals_the_golden():
    with open(os.path.join(HERE, "golden", "enter_snapshot.json")) as f:
        g = json.load(f)
    assert g["script"] == esm.golden_script()
    gen.check_conditions(g["script"], g["answers"])
    got = esm.replay(g["script"])
    assert len(got) == len(g["answers"])
    snaps = [ln for ln in g["script"] if ln.startswith("S ")]
    for k, (a, b) in enumerate(zip(got, g["answers"])):
        assert a == b, (k, snaps[k])
