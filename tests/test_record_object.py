"""CPU: object (NFGUID) record columns.  The entry points exist in libnfgpu.so and refuse a null world;
nfk_jit_preview_rec (no GPU needed) takes a schema with an object column and refuses a record op and
a cell guard on a half; the model of the reference's NFCRecord with NFGUID columns
(tests/record_object_model.py) on a record small enough to answer by hand, and on the answers
recorded from the compiled reference (tests/golden/record_object.json)."""
import ctypes
import json
import os

import numpy as np

from noahgameframe_amd import kernel
from noahgameframe_amd import workload as wl
from tests import record_object_model as rom
from tests.record_find_model import FLOAT, INT, f64_bits
from tests.record_object_model import EV_ADD, EV_COVER, EV_DEL, EV_UPDATE, NULL_OBJECT, OBJECT, ORecord


def test_library_exports_the_object_record_calls():
    lib = kernel.load_library()
    one = np.zeros(1, np.int64)
    i32 = np.zeros(1, np.int32)
    m = np.zeros(1, np.uint64)
    p = kernel._p
    for name, args in (("nfk_set_record_objects", (1, p(one), p(one), p(i32), p(i32), p(i32), p(one), p(one))),
                       ("nfk_get_record_objects", (1, p(one), p(one), p(i32), p(i32), p(i32), p(one), p(one))),
                       ("nfk_find_objects", (1, p(one), p(one), p(i32), p(i32), p(one), p(one), p(m))),
                       ("nfk_find_objects_obj", (1, p(i32), p(i32), p(i32), p(one), p(one), p(m))),
                       ("nfk_read_rec_events_obj", (p(m), p(m)))):
        assert hasattr(lib, name), name
        assert getattr(lib, name)(None, *args) == -1, name   # NFK_ERR_ARG
        assert b"null" in lib.nfk_last_error(), name
    assert (kernel.REC_INT, kernel.REC_F64, kernel.REC_OBJ_DATA, kernel.REC_OBJ_HEAD) == (0, 1, 2, 3)
    assert ctypes.sizeof(kernel.Outputs) % 8 == 0 and hasattr(kernel.Outputs, "re_new_h")


def _preview(ops, col_types, rows=8, cols=4):
    """nfk_jit_preview_rec without a compile: (status, ok) for one kind over one record"""
    lib = kernel.load_library()
    n_int, n_flt = 2, 1
    flags = np.zeros((2, n_int + n_flt), np.uint8)
    prog = np.zeros((1, 8), wl.OP_DTYPE)
    for i, op in enumerate(ops):
        for k, v in op.items():
            prog[0, i][k] = v
    n_ops = np.array([len(ops)], np.int32)
    ct = np.zeros((1, 16), np.uint8)
    ct[0, :len(col_types)] = col_types
    ok = ctypes.c_int32(-1)
    src = ctypes.create_string_buffer(1 << 20)
    msg = ctypes.create_string_buffer(4096)
    p = kernel._p
    rc = lib.nfk_jit_preview_rec(n_int, n_flt, 2, 1, p(flags), p(prog), p(n_ops), 1, p(np.array([rows], np.int32)),
                                 p(np.array([cols], np.int32)), p(ct), 0, ctypes.byref(ok), src, len(src), msg, len(msg))
    return rc, ok.value


def test_jit_preview_takes_object_columns_and_refuses_ops_on_halves():
    iadd = dict(code=1, dst=0, a=1, b=0, c=100)                       # IADD_CLAMP on int property 0
    types = [kernel.REC_INT, kernel.REC_OBJ_DATA, kernel.REC_OBJ_HEAD, kernel.REC_F64]
    assert _preview([iadd], types) == (0, 1)
    cell = lambda col: (0 << 10) | (3 << 4) | col                     # NFK_GUARD_CELL_ID(0, 3, col)
    guard = lambda col: dict(code=1, flags=8 | 16, dst=0, a=1, b=0, c=100, guard=cell(col))
    assert _preview([guard(0)], types) == (0, 1)                      # a guard on the int cell
    for col in (1, 2):                                                # ... on either half: refused
        assert _preview([guard(col)], types)[0] == -1
    # a record op on a half: refused; on the int / f64 column beside it: taken
    assert _preview([dict(code=4, dst=(0 << 8) | 0, a=1, b=0, c=9)], types) == (0, 1)
    for col in (1, 2):
        assert _preview([dict(code=4, dst=(0 << 8) | col, a=1, b=0, c=9)], types)[0] == -1
        assert _preview([dict(code=5, dst=(0 << 8) | col, a=f64_bits(1.0), b=f64_bits(0.5))], types)[0] == -1
    # a data half without its head half, a head half alone, an unknown type
    for bad in ([2, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 2], [3, 2, 0, 0], [2, 2, 3, 0], [4, 0, 0, 0]):
        assert _preview([iadd], bad)[0] == -1, bad


def _hero():
    # 5 rows x (NFGUID, int, NFGUID); rows 0, 1, 3 used
    r = ORecord(5, "OIO")
    for row, v in {0: ((3, 9), 1, (0, 0)), 1: ((3, 9), 2, (4, 9)), 3: ((4, 9), 2, (3, 9))}.items():
        assert r.add_row(row, v) == row
    return r


def test_model_by_hand():
    r = _hero()
    assert r.types == [2, 3, 0, 2, 3] and r.phys == [0, 2, 3] and r.cols == 5 and r.lcols == 3
    assert [e[0] for e in r.events] == [EV_ADD] * 3
    out = []
    assert r.find_object(0, (3, 9), out) == 2 and out == [0, 1]
    assert r.find_object(2, (3, 9), out) == 3 and out == [0, 1, 3]            # appended; the total size
    # one half equal is no hit
    assert r.omask(0, (3, 8)) == 0 and r.omask(0, (9, 3)) == 0 and r.omask(0, (4, 9)) == 1 << 3
    # NULL_OBJECT finds the used rows that hold it
    out = []
    assert r.find_object(2, NULL_OBJECT, out) == 1 and out == [0]
    # SetObject: refused on an unused row, an invalid cell, a column of another type, an equal value
    n = len(r.events)
    assert not r.set_object(2, 0, (5, 5)) and not r.set_object(5, 0, (5, 5)) and not r.set_object(0, 3, (5, 5))
    assert not r.set_object(0, 1, (5, 5)) and not r.set_object(0, 0, (3, 9)) and len(r.events) == n
    assert not r.set_int(0, 0, 7) and r.set_int(0, 1, 7) and r.events[-1] == (EV_UPDATE, 0, 1, (0, 1), (0, 7))
    # only the head half changes; then only the data half; one Update each, with both halves
    assert r.set_object(0, 0, (4, 9)) and r.events[-1] == (EV_UPDATE, 0, 0, (3, 9), (4, 9))
    assert r.set_object(0, 0, (4, 8)) and r.events[-1] == (EV_UPDATE, 0, 0, (4, 9), (4, 8))
    assert r.get_object(0, 0) == (4, 8) and int(r.cells[0, 0]) == 8 and int(r.cells[1, 0]) == 4   # data, then head
    assert r.get_object(2, 0) == NULL_OBJECT and r.get_object(0, 1) == NULL_OBJECT and r.get_object(9, 0) == NULL_OBJECT
    # negative halves are bit patterns
    assert r.set_object(1, 2, (-1, -2)) and r.get_object(1, 2) == (-1, -2) and r.omask(2, (-1, -2)) == 2
    assert int(r.cells[3, 1]) == (1 << 64) - 2 and int(r.cells[4, 1]) == (1 << 64) - 1
    # a removed row keeps its cells: the stale NFGUID is not found; re-added without values it holds NULL_OBJECT
    assert r.remove(3) and r.events[-1][0] == EV_DEL and r.omask(0, (4, 9)) == 0
    assert r.add_row(-1) == 2 and r.add_row(3) == 3 and r.events[-1][:2] == (EV_ADD, 3)
    assert r.add_row(3, [(1, 1), 0, (2, 2)]) == 3 and r.events[-1][:2] == (EV_COVER, 3)
    assert r.omask(0, NULL_OBJECT) == 1 << 2 and r.query_row(2) == [(0, 0), 0, (0, 0)]
    assert r.query_row(3) == [(1, 1), 0, (2, 2)] and r.query_row(4) is None
    # FindRowByColValue: var's element 0 gives the type, the value is read at index nCol
    q = lambda col, var: (lambda l: (r.find_row_by_col_value(col, var, l), l))([])
    assert q(0, [(OBJECT, (1, 1))]) == (1, [3])
    assert q(2, [(OBJECT, (1, 1))]) == (2, [0, 2])                     # var[2] past the end: NULL_OBJECT
    assert q(2, [(OBJECT, (1, 1)), (INT, 0), (OBJECT, (2, 2))]) == (1, [3])
    assert q(2, [(OBJECT, (1, 1)), (INT, 0), (INT, 2)]) == (2, [0, 2])  # var[2] of another type: NULL_OBJECT
    assert q(1, [(OBJECT, (1, 1))]) == (-1, []) and q(0, [(INT, 1)]) == (-1, []) and q(0, []) == (-1, [])
    assert q(1, [(INT, 9), (INT, 7)]) == (1, [0]) and q(3, [(INT, 1)]) == (-1, [])
    assert r.find_object(1, (0, 0), []) == -1 and r.find_int(0, 0, []) == -1 and r.find_float(1, 0.0, []) == -1
    # Clear removes from the last row to the first
    n = len(r.events)
    r.clear()
    assert [e[:2] for e in r.events[n:]] == [(EV_DEL, 3), (EV_DEL, 2), (EV_DEL, 1), (EV_DEL, 0)]


def test_coalescing_rule_by_hand():
    """row events first in call order, then one Update per changed cell in (row, col) order: first
    old, last new, dropped when all 128 bits are equal"""
    r = _hero()
    r.events.clear()
    assert r.set_object(1, 2, (9, 9)) and r.set_object(1, 2, (4, 9))          # away and back: no event
    assert r.set_object(1, 0, (3, 8)) and r.set_object(1, 0, (5, 8))          # first old, last new
    assert r.set_int(0, 1, 5) and r.set_object(0, 2, (0, 1))
    assert r.remove(3) and r.add_row(3, [(7, 7), 1, (0, 0)]) == 3 and r.set_object(3, 0, (7, 8))
    assert rom.coalesce(r.events) == [
        (EV_DEL, 3, 0, NULL_OBJECT, NULL_OBJECT), (EV_ADD, 3, 0, NULL_OBJECT, NULL_OBJECT),
        (EV_UPDATE, 0, 1, (0, 1), (0, 5)), (EV_UPDATE, 0, 2, (0, 0), (0, 1)),
        (EV_UPDATE, 1, 0, (3, 9), (5, 8)), (EV_UPDATE, 3, 0, (7, 7), (7, 8))]


def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_object.json")) as f:
        return json.load(f)


def test_model_equals_the_compiled_reference():
    """every return value, hook event and find / QueryRow / GetObject answer the compiled reference
    gave over the golden script (tests/golden/record_object.json, written by
    tests/golden/gen_record_object_golden.py), by the model, call for call"""
    g = golden()
    script, answers = g["script"], g["answers"]
    assert script == rom.golden_script()
    got = rom.replay(script)
    assert len(got) == len(answers)
    for k, (a, b) in enumerate(zip(got, answers)):
        assert a == b, (k, a, b)
    # the golden world: a few dozen objects, four windows, the four layouts (Edge: halves at physical 14, 15)
    assert script[:5] == ["REC Hero 16 OIF", "REC Team 64 O", "REC Pair 5 OO", "REC Edge 20 IIIIIIIIIIIIIIO", "OBJ 24"]
    assert script.count("X") == 4
    assert rom.physical_types("I" * 14 + "O")[14:] == [2, 3] and ORecord(20, "I" * 14 + "O").phys[14] == 14
    ops = {ln.split()[0] for ln in script}
    assert {"SO", "SI", "RM", "AR", "CL", "FO", "FO+", "FI+", "FV", "QR", "GO"} <= ops
    rom.check_conditions(script, answers)
