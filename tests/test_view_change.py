"""CPU: tests/view_change_model.py (the visit rules of nfk_view_changes and the composition of the
reference's OnObjectListEnter / OnObjectListLeave calls from a visit's lists) against
tests/golden/view_change.json, the recorded calls of the compiled reference (NFCKernelModule +
NFCSceneAOIModule, tests/cpp/view_change_ref.cpp) over the golden script — line by line — and the
cases that script is there for."""
import json
import os

from tests import view_change_model as vcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "view_change.json")))


def test_golden_script_is_the_models():
    assert GOLD["script"] == vcm.golden_script()


def test_model_replays_the_reference_line_by_line():
    lines, _ = vcm.replay_script(GOLD["script"])
    assert len(lines) == len(GOLD["lines"])
    for i, (got, want) in enumerate(zip(lines, GOLD["lines"])):
        assert got == want, f"call {i}"


def test_script_holds_its_cases():
    _, cases = vcm.replay_script(GOLD["script"])   # (asserts per switch that only Players move)
    assert cases >= vcm.GOLDEN_CASES, vcm.GOLDEN_CASES - cases
    # the reference released the old group on every group leave (AOI:389-393): the harness recorded and
    # neutralised each one
    leaves = sum(1 for ln in GOLD["script"] if ln.startswith("SW "))
    assert 0 < len(GOLD["released"]) <= leaves
    # empty lists occur on both sides: AOI:506's Leave with nothing in it, AOI:326's with nobody told
    assert any(ln.endswith(" :") for ln in GOLD["lines"]) and any(ln.startswith("L :") for ln in GOLD["lines"])
    assert any(ln.startswith("E :") for ln in GOLD["lines"])    # AOI:508's test on the list with self


def test_visits_of_every_kind():
    v = vcm.visits_of
    assert v(vcm.VC_SWITCH, 1, 2, 1, 3) == [(vcm.GROUP_LEAVE, 1, 2), (vcm.GROUP_ENTER, 1, 3)]
    assert v(vcm.VC_SWITCH, 1, 0, 1, 3) == [(vcm.GROUP_ENTER, 1, 3)]
    assert v(vcm.VC_SWITCH, 1, 2, 2, 0) == [(vcm.GROUP_LEAVE, 1, 2), (vcm.SCENE_LEAVE, 1, 0), (vcm.SCENE_ENTER, 2, 0)]
    assert len(v(vcm.VC_SWITCH, 1, 2, 2, 4)) == 4
    assert v(vcm.VC_DESTROY, 0, 0, 0, 0) == [] and v(vcm.VC_DESTROY, 1, 0, 0, 0) == [(vcm.WHY_DESTROY, 1, 0)]
    assert v(vcm.VC_CREATE, 0, 0, 2, 3) == [(vcm.SCENE_ENTER, 2, 0), (vcm.GROUP_ENTER, 2, 3)]
    assert v(vcm.VC_EXPORT, 1, 2, 0, 0) == [(vcm.GROUP_LEAVE, 1, 2), (vcm.SCENE_LEAVE, 1, 0)]
