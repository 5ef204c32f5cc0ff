"""Writes tests/golden/scene_query.json: the reference's own answers to the scene queries over
tests.scene_query_model.golden_world().

Run by hand on a machine that has the reference tree (REF, default /root/reference); not part of the
build.  tests/cpp/scene_query_ref.cpp is compiled against the reference's sources where they lie (the
file list of oracle/Makefile.adapter's logic_session_ref, with oracle/ref_server.hpp and oracle/nfio.h)
into oracle/_ref/scene_query_ref and run on the world; only its recorded answers are kept.

    python tests/golden/gen_scene_query_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from noahgameframe_amd import nfio  # noqa: E402
from tests import scene_query_model as sqm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
CORE = ["NFCDataList", "NFCProperty", "NFCPropertyManager", "NFCRecord", "NFCRecordManager", "NFCObject",
        "NFCComponentManager", "NFCMemManager", "NFMemoryCounter"]
KERNEL = ["NFCKernelModule", "NFCSceneAOIModule", "NFCEventModule", "NFCScheduleModule"]
CONFIG = ["NFCClassModule", "NFCElementModule"]


def parse(stdout):
    """the Q lines of scene_query_ref / scene_query_plugin -> {(frame, phase): [[call, a, b, c, d, ret, list]]}"""
    out = {}
    for ln in stdout.splitlines():
        if not ln.startswith("Q "):
            continue
        head, lst = ln.split(":")
        f = head.split()
        out.setdefault((int(f[1]), f[2]), []).append(
            [f[3], int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[9]), [int(x) for x in lst.split()]])
    return out


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "scene_query_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = ([os.path.join(REF, "NFComm", "NFCore", n + ".cpp") for n in CORE] +
           [os.path.join(REF, "NFComm", "NFKernelPlugin", n + ".cpp") for n in KERNEL] +
           [os.path.join(REF, "NFComm", "NFConfigPlugin", n + ".cpp") for n in CONFIG])
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I", REF, "-I", os.path.join(REF, "Dependencies"),
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "scene_query_ref.cpp"), *src, "-lpthread"], check=True)
    w = sqm.golden_world()
    with tempfile.TemporaryDirectory() as d:
        wp = os.path.join(d, "w.nfio")
        nfio.write(wp, w)
        run = subprocess.run([exe, wp], capture_output=True, text=True, check=True)
    ans = parse(run.stdout)
    n_ticks = int(w["cfg"][7])
    frames = [ans[(t, "ref")] for t in range(n_ticks)]
    path = os.path.join(ROOT, "tests", "golden", "scene_query.json")
    with open(path, "w") as f:
        json.dump({"world": "tests.scene_query_model.golden_world()", "frames": frames}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {sum(len(fr) for fr in frames)} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
