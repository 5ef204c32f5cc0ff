"""Writes tests/golden/view_change.json: the reference's own OnObjectListEnter / OnObjectListLeave calls
over tests.view_change_model.golden_script().

Run by hand on a machine that has the reference tree (REF, default /root/reference); not part of the
build.  tests/cpp/view_change_ref.cpp is compiled against the reference's sources where they lie (its
NFCKernelModule and NFCSceneAOIModule, the AOI module's common callbacks left registered) into
oracle/_ref/view_change_ref and run on the script; only the script and its recorded answers are kept.

    python tests/golden/gen_view_change_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import view_change_model as vcm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
CORE = ["NFCDataList", "NFCProperty", "NFCPropertyManager", "NFCRecord", "NFCRecordManager", "NFCObject",
        "NFCComponentManager", "NFCMemManager", "NFMemoryCounter"]
KERNEL = ["NFCKernelModule", "NFCSceneAOIModule", "NFCEventModule", "NFCScheduleModule"]
CONFIG = ["NFCClassModule", "NFCElementModule"]


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "view_change_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = ([os.path.join(REF, "NFComm", "NFCore", n + ".cpp") for n in CORE] +
           [os.path.join(REF, "NFComm", "NFKernelPlugin", n + ".cpp") for n in KERNEL] +
           [os.path.join(REF, "NFComm", "NFConfigPlugin", n + ".cpp") for n in CONFIG])
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I", REF, "-I", os.path.join(REF, "Dependencies"),
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "view_change_ref.cpp"), *src, "-lpthread"], check=True)
    script = vcm.golden_script()
    # the script moves Players only: NFCKernelModule::SwitchScene files every mover under the player
    # lists (KM:929, 945), which the device does not reproduce (replay_script asserts it per switch)
    _, cases = vcm.replay_script(script)
    assert cases >= vcm.GOLDEN_CASES, vcm.GOLDEN_CASES - cases
    with tempfile.TemporaryDirectory() as d:
        sp = os.path.join(d, "script.txt")
        with open(sp, "w") as f:
            f.write("\n".join(script) + "\n")
        run = subprocess.run([exe, sp], capture_output=True, text=True, check=True)
    out = run.stdout.splitlines()
    lines = [ln for ln in out if ln[:1] in "EL"]
    released = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("R ")]
    assert lines   # (the class module prints a line of its own: everything but E / L / R lines is dropped)
    path = os.path.join(ROOT, "tests", "golden", "view_change.json")
    with open(path, "w") as f:
        json.dump({"world": "tests.view_change_model.golden_script()", "script": script, "lines": lines,
                   "released": released}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(lines)} calls, {len(released)} neutralised releases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
