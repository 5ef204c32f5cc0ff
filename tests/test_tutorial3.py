"""The reference's Tutorial3 (Tutorial/Tutorial3/HelloWorld3Module.cpp, Tutorial3Plugin.cpp) compiled unchanged
where it lies and loaded by a server (tests/cpp/tutorial3_session.cpp) once with the reference's own
NFKernelPlugin and once with the reference-side GPU plugin (integration/NFGPUKernelPlugin.cpp) in its place:
config[0]'s named workload ("Tutorial3 heartbeat/property-callback demo scaled to 10k NPC objects") through the
drop-in without a restatement.  Everything the tutorial prints — its class callbacks for every object, OnEvent
for the DoEvent calls, OnHeartBeat's count and time distance (NFGetTime on the session's clock) for every fired
heartbeat in the walk's order, its property callbacks — must be equal, frame by frame.  The reference's run at
10k objects takes about a minute, so the GPU test compares with per-frame digests of it
(tests/golden/tutorial3_10k.json, tests/golden/gen_tutorial3_golden.py)."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "oracle", "_ref", "tutorial3_session")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "tutorial3_session_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tutorial3_10k.json")
ARGS_10K = ("10000", "24", "500")  # objects, frames, tick ms


def run(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def frames(text):
    """the tutorial's output split at the session's frame lines: {"setup": [...], 0: [...], ...}"""
    out, cur = {"setup": []}, "setup"
    for ln in text.splitlines():
        if ln.startswith("== frame "):
            cur = int(ln.split()[2])
            out[cur] = []
        elif ln.startswith("== "):
            continue
        else:
            out[cur].append(ln)
    return out


def digests(text):
    return {str(k): [len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()] for k, v in frames(text).items()}


def test_tutorial3_reference_session_runs_the_tutorial():
    """CPU: the unchanged tutorial on the reference's modules prints what HelloWorld3Module.cpp does — Init,
    AfterInit, its own object's property callbacks and OnEvent (:68-100), a class callback per object, OnEvent
    for the DoEvent calls, and OnHeartBeat (5 s x 10) with the count going down."""
    if not os.path.exists(REF_EXE):
        pytest.skip("tutorial3_session_ref not built (needs /root/reference at build time)")
    f = frames(run(REF_EXE, ("300", "24", "500")))
    setup = f["setup"]
    assert "Hello, world3, Init" in setup and "Hello, world3, AfterInit" in setup
    assert "OnPropertyCallBackEvent Property: World OldValue: 0 NewValue: 1111" in setup
    assert "OnEvent EventID: 1 self: 10 argList: 100  200" in setup
    body = [ln for t in range(24) for ln in f[t]]
    assert sum("OnClassCallBackEvent ClassName: Player" in ln for ln in body) >= 300 * 5
    hb = [ln for ln in body if ln.startswith("strHeartBeat: 5 Count: ")]
    assert len(hb) > 300 and any("Count: 8" in ln for ln in hb)
    assert sum(ln.startswith("OnEvent EventID: 1 self: ") for ln in body) > 20


@pytest.mark.gpu
def test_tutorial3_unchanged_through_the_gpu_plugin_small(gpu_available):
    """300 objects: the GPU plugin's run equals the reference's line for line."""
    if not (os.path.exists(GPU_EXE) and os.path.exists(REF_EXE)):
        pytest.skip("tutorial3_session not built (needs /root/reference at build time)")
    got, ref = frames(run(GPU_EXE, ("300", "24", "500"))), frames(run(REF_EXE, ("300", "24", "500")))
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k] == ref[k], (k, [x for x in got[k] if x not in ref[k]][:5], [x for x in ref[k] if x not in got[k]][:5])


@pytest.mark.gpu
def test_tutorial3_unchanged_through_the_gpu_plugin_10k(gpu_available):
    """config[0]'s scale, 10k objects: the GPU plugin's output equals the reference's, frame by frame
    (digests of the reference's run)."""
    if not os.path.exists(GPU_EXE):
        pytest.skip("tutorial3_session not built (needs /root/reference at build time)")
    gold = json.load(open(GOLDEN))
    assert gold["args"] == list(ARGS_10K)
    dg = digests(run(GPU_EXE, ARGS_10K))
    bad = [k for k in gold["frames"] if dg.get(k) != gold["frames"][k]]
    assert not bad, [(k, dg.get(k), gold["frames"][k]) for k in bad[:5]]
    assert sum(v[0] for v in gold["frames"].values()) > 90000
