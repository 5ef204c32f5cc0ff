"""Resource calls on the CPU: the model (tests/resource_call_model.py) against the compiled reference's
recorded answers (tests/golden/resource_calls.json, written by tests/golden/gen_resource_calls_golden.py),
and the op table's unit cases."""
import json
import os

import pytest

from tests import resource_call_model as rcm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resource_calls.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_script_is_the_models(golden):
    assert golden["script"] == rcm.golden_script()
    assert golden["props"] == rcm.PROPS
    assert len(golden["answers"]) == sum(1 for ln in golden["script"] if ln.split()[0] not in ("BASE", "OBJ", "X"))


def test_model_replays_the_reference_line_by_line(golden):
    got = rcm.replay(golden["script"])
    assert len(got) == len(golden["answers"])
    calls = [ln for ln in golden["script"] if ln.split()[0] not in ("BASE", "OBJ", "X")]
    for k, (g, a) in enumerate(zip(got, golden["answers"])):
        assert g == a, (k, calls[k], g, a)


def test_conditions_hold_on_the_committed_golden(golden):
    n = rcm.check_conditions(golden["script"], golden["answers"])
    assert set(n) == set(rcm.CONDITIONS)


def test_conditions_miss_a_dropped_case(golden):
    """check_conditions is no formality: without the AddHP-on-zero line it fails"""
    script = [ln for ln in golden["script"] if ln != "AddHP 0 5"]
    answers = rcm.replay(script)
    with pytest.raises(AssertionError):
        rcm.check_conditions(script, answers)


B62 = 1 << 62
UNIT = [
    # op, cur, max, v -> (ret, new)
    (rcm.GAIN_ALIVE, 5, 10, 0, (0, None)), (rcm.GAIN_ALIVE, 5, 10, -1, (0, None)), (rcm.GAIN_ALIVE, 0, 10, 3, (1, None)),
    (rcm.GAIN_ALIVE, -4, 10, 3, (1, None)), (rcm.GAIN_ALIVE, 5, 10, 3, (1, 8)), (rcm.GAIN_ALIVE, 5, 10, 5, (1, 10)),
    (rcm.GAIN_ALIVE, 5, 10, 6, (1, 10)), (rcm.GAIN_ALIVE, 50, 10, 1, (1, 10)), (rcm.GAIN_ALIVE, 5, -3, 1, (1, -3)),
    (rcm.GAIN_ALIVE, B62, 2 * B62 - 1, B62 - 1, (1, 2 * B62 - 1)),
    (rcm.GAIN_CAP, 0, 10, 3, (1, 3)), (rcm.GAIN_CAP, -7, 10, 3, (1, -4)), (rcm.GAIN_CAP, 9, 10, 3, (1, 10)),
    (rcm.GAIN_CAP, 9, 10, 0, (0, None)), (rcm.GAIN_CAP, 0, 0, 5, (1, 0)),
    (rcm.GAIN, 0, 0, 5, (0, 5)), (rcm.GAIN, 7, 0, -1, (0, None)), (rcm.GAIN, 7, 0, 0, (0, None)),
    (rcm.GAIN, B62, 0, B62 - 1, (0, 2 * B62 - 1)),
    (rcm.SPEND_ALIVE, 10, 0, 10, (1, 0)), (rcm.SPEND_ALIVE, 10, 0, 11, (0, None)), (rcm.SPEND_ALIVE, 0, 0, 0, (0, None)),
    (rcm.SPEND_ALIVE, 10, 0, 0, (1, 10)), (rcm.SPEND_ALIVE, 10, 0, -5, (1, 15)), (rcm.SPEND_ALIVE, -3, 0, -5, (0, None)),
    (rcm.SPEND_ALIVE, B62, 0, -(B62 - 1), (1, 2 * B62 - 1)),
    (rcm.SPEND, 10, 0, 10, (1, 0)), (rcm.SPEND, 10, 0, 11, (0, None)), (rcm.SPEND, 10, 0, 0, (0, None)),
    (rcm.SPEND, 10, 0, -1, (0, None)), (rcm.SPEND, 0, 0, 1, (0, None)), (rcm.SPEND, -B62, 0, 1, (0, None)),
    (rcm.ENOUGH, 10, 0, 10, (1, None)), (rcm.ENOUGH, 10, 0, 11, (0, None)), (rcm.ENOUGH, 0, 0, 0, (0, None)),
    (rcm.ENOUGH, 1, 0, -B62, (1, None)), (rcm.ENOUGH, -1, 0, -5, (0, None)),
    (rcm.FILL, 3, 10, 99, (1, 10)), (rcm.FILL, 3, 0, 0, (0, None)), (rcm.FILL, 3, -2, 0, (0, None)),
    (rcm.FILL, 10, 10, 0, (1, 10)),
]


@pytest.mark.parametrize("op,cur,mx,v,want", UNIT)
def test_rule_unit_cases(op, cur, mx, v, want):
    assert rcm.rule(op, cur, mx, v) == want


def test_adjust_applies_in_order_and_records_every_set():
    w = {(0, 0): 10, (0, 3): 20}
    calls = [(0, rcm.SPEND_ALIVE, 0, -1, 4), (0, rcm.GAIN_ALIVE, 0, 3, 100), (0, rcm.FILL, 0, 3, 0),
             (0, rcm.ENOUGH, 0, -1, 20), (1, rcm.GAIN, 6, -1, 5), (0, rcm.GAIN, 3, -1, 1), (0, rcm.GAIN_ALIVE, 0, 3, 9)]
    rets, sets = rcm.adjust(w, calls)
    assert rets == [3, 3, 3, 1, 2, 2, 3]          # (a Set of the value already held is still a Set)
    assert sets == [(0, 0, 6), (0, 0, 20), (0, 0, 20), (1, 6, 5), (0, 3, 21), (0, 0, 21)]
    assert w == {(0, 0): 21, (0, 3): 21, (1, 6): 5}


def test_named_methods_cover_the_seventeen():
    assert len(rcm.METHODS) == 17
    for name, calls in rcm.METHODS.items():
        for op, d, b in calls:
            assert (b is not None) == (op in rcm.TAKES_BOUND), name
    assert rcm.method_return("FullHPMP", [0, 0]) == 1
    assert rcm.method_return("FullSP", [0]) == 0
