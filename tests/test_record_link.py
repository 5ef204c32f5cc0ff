"""CPU: property links (nfk_link_record) — tests/record_link_model.py by hand on a 3 x 2 record, its
window rule, the model replaying the answers recorded from the compiled reference
(tests/golden/record_link.json), the cases that golden holds, and the entry point: declared in
nfgpu.h, exported, bound in kernel.py, refusing a null world."""
import ctypes
import json
import os
import re

import numpy as np

from noahgameframe_amd import kernel
from tests import record_link_model as rlm
from tests.parity import ROOT
from tests.record_link_model import LinkRecord

MAXHP, ATK = 4, 9       # (any two int property ids)


def _rec():
    """3 rows x 2 columns, the link over the first 2 rows: row 2 never counts"""
    return LinkRecord(3, 2, rows_l=2, col_pid=[MAXHP, ATK], props={MAXHP: 0, ATK: 0})


def test_model_by_hand():
    r = _rec()
    # AddRow names column 0 only: ATK stays stale though column 1 holds 7
    assert r.add_row(0, [10, 7]) == 0
    assert r.props == {MAXHP: 10, ATK: 0} and r.sets == [(MAXHP, 0, 10)]
    # a Set on an unused row is refused and raises nothing
    assert not r.set_int(1, 1, 5) and r.n_events == 1
    # an accepted Set names its column: ATK catches up
    assert r.set_int(0, 1, 8) and r.props[ATK] == 8
    # an unchanged Set raises nothing
    n = r.n_events
    assert not r.set_int(0, 1, 8) and r.n_events == n
    assert r.add_row(-1, [5, 1]) == 1 and r.props[MAXHP] == 15 and r.props[ATK] == 8     # (stale again: 9 by the cells)
    assert r.link_sum(1) == 9
    # a row outside the link's rows: its event fires, its cells do not count
    assert r.add_row(2, [100, 100]) == 2 and r.props[MAXHP] == 15
    assert r.set_int(2, 1, 50) and r.props[ATK] == 9       # (the event named column 1: the stale value goes)
    # Remove: the event comes before the row goes, so the removed row still counts
    r.set_int(1, 0, 6)
    assert r.props[MAXHP] == 16
    assert r.remove(1) and r.props[MAXHP] == 16 and r.link_sum(0) == 10
    # the next event of column 0 sees the row gone
    assert r.set_int(0, 0, 11) and r.props[MAXHP] == 11
    # a Swap names the column whose index is its TARGET ROW: target 1 -> column 1, summed after the exchange
    r.props[ATK] = -1
    assert r.swap_row_info(0, 1)
    assert r.used == 0b110 and r.props[ATK] == 8 and r.props[MAXHP] == 11      # (row 0 is unused now; MAXHP is stale)
    # target 2 is no column: nothing
    n = len(r.sets)
    assert r.swap_row_info(1, 2) and len(r.sets) == n
    # origin unused: refused, no event
    n = r.n_events
    assert not r.swap_row_info(0, 1) and r.n_events == n
    # Clear: Remove from the last row down, each step an event of column 0 before its row goes; the
    # last step sums the lowest used row alone — if the link reaches it
    r = _rec()
    r.add_row(0, [3, 0])
    r.add_row(1, [4, 0])
    r.add_row(2, [9, 0])
    assert r.props[MAXHP] == 7
    r.props[MAXHP] = 99
    r.clear()
    assert r.used == 0
    assert r.props[MAXHP] == 3 and r.sets[-2:] == [(MAXHP, 99, 7), (MAXHP, 7, 3)]


def test_model_int32_edges():
    r = LinkRecord(2, 1, rows_l=2, col_pid=[MAXHP], props={MAXHP: 0})
    r.add_row(0, [(1 << 32) + 5])                       # truncated to int32 before the add
    assert r.props[MAXHP] == 5
    r.set_int(0, 0, -(1 << 31))
    assert r.props[MAXHP] == -(1 << 31)
    r.add_row(1, [-1])                                  # the add wraps modulo 2^32 (pinned on the model only)
    assert r.props[MAXHP] == (1 << 31) - 1
    r.set_int(0, 0, (1 << 31) - 1)
    r.set_int(1, 0, 1)
    assert r.props[MAXHP] == -(1 << 31)
    r.set_int(0, 0, -(1 << 63))                         # low 32 bits 0
    assert r.props[MAXHP] == 1


def test_model_window_rule():
    """one event per property, frame-start -> final, dropped when equal, property-id order"""
    r = _rec()
    r.add_row(0, [1, 1])
    r.set_int(0, 1, 2)
    assert r.frame_events() == [(MAXHP, 0, 1), (ATK, 0, 2)]
    r.set_int(0, 0, 5)
    r.set_int(0, 0, 1)              # back to the frame-start value: no event
    r.set_int(0, 1, 3)
    assert [s[0] for s in r.sets] == [MAXHP, MAXHP, ATK]
    assert r.frame_events() == [(ATK, 2, 3)]
    assert r.frame_events() == []


def test_random_calls_reach_every_kind():
    rng = np.random.default_rng(5)
    r = LinkRecord(7, 16, rows_l=7, col_pid=list(range(16)))
    kinds = {}
    for _ in range(400):
        c = rlm.random_call(rng, r)
        res = r.apply(c)
        kinds[c[0]] = kinds.get(c[0], 0) + int(res is not False and res != -1)
    assert all(kinds.get(k, 0) > 0 for k in ("set", "add", "rm", "swap", "clear")), kinds
    assert len(r.sets) > 50


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "record_link.json")) as f:
        return json.load(f)


def test_model_replays_the_reference():
    """the compiled NFCPropertyModule's answers, line for line: every object's linked properties right
    after CreateObject, then per call the return value and the object's linked properties"""
    g = _golden()
    script, answers = g["script"], g["answers"]
    assert script == rlm.golden_script(), "tests/golden/record_link.json is not golden_script()'s world"
    created, got = rlm.replay(script)
    assert created == g["created"]
    calls = [ln for ln in script if ln.split()[0] not in ("SHAPE", "TAGS", "BASE", "OBJ", "X")]
    assert len(got) == len(answers) == len(calls)
    for k, (a, b) in enumerate(zip(got, answers)):
        assert a == b, (k, calls[k], a, b)


def test_golden_conditions():
    g = _golden()
    n = rlm.check_conditions(g["script"], g["answers"])
    assert set(n) == set(rlm.CONDITIONS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "record_link.json")) < 128 * 1024
    # a level-up rewrites row 0 of every column: its line carries one base value per column
    lv = [ln.split() for ln in g["script"] if ln.startswith("LV ")]
    assert lv and all(len(f) == 3 + rlm.GOLDEN_COLS for f in lv)


def test_library_and_python_know_the_call():
    """nfk_link_record: declared in nfgpu.h, exported, bound in kernel.py with the header's
    parameters, refusing a null world"""
    src = open(os.path.join(ROOT, "include", "nfgpu.h")).read()
    m = re.search(r"^int\s+nfk_link_record\((.*?)\);", src, re.M | re.S)
    assert m, "nfgpu.h does not declare nfk_link_record"
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ["void* world", "int32_t rec", "int32_t rows", "const int32_t* col_pid", "int32_t mode"], params
    assert re.search(r"^#define NFK_LINK_SUM32 0$", src, re.M) and kernel.LINK_SUM32 == 0
    lib = kernel.load_library()
    assert hasattr(lib, "nfk_link_record")
    want = [ctypes.c_void_p if "*" in p else ctypes.c_int32 for p in params]
    assert list(lib.nfk_link_record.argtypes) == want and lib.nfk_link_record.restype is ctypes.c_int
    pid = np.zeros(16, np.int32)
    assert lib.nfk_link_record(None, 0, 1, kernel._p(pid), kernel.LINK_SUM32) == -1     # NFK_ERR_ARG
    assert b"null" in lib.nfk_last_error()
    assert callable(getattr(kernel.NFKernelModule, "link_record", None))
