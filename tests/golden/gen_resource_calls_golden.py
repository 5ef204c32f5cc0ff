"""Regenerate tests/golden/resource_calls.json: the script of tests/resource_call_model.py
(golden_script()) replayed on the compiled reference — NFCPropertyModule.cpp with the reference's kernel,
class and element modules, built where they lie into oracle/_ref/resource_calls_ref
(tests/cpp/resource_calls_ref.cpp) — and its answers: per call line the return value and the eight
properties (HP MP SP MAXHP MAXMP MAXSP Gold Money) of the line's object after the call.  The generation
fails when one of the model's CONDITIONS is missing from the answers.  Needs the reference tree (REF,
default /root/reference).

usage: python tests/golden/gen_resource_calls_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resource_call_model as rcm  # noqa: E402


def build(ref):
    out = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "resource_calls_ref")
    core = ["NFCDataList", "NFCProperty", "NFCPropertyManager", "NFCRecord", "NFCRecordManager", "NFCObject",
            "NFCComponentManager", "NFCMemManager", "NFMemoryCounter"]
    src = ([os.path.join(ref, "NFServer", "NFGameServerPlugin", "NFCPropertyModule.cpp")] +
           [os.path.join(ref, "NFComm", "NFCore", n + ".cpp") for n in core] +
           [os.path.join(ref, "NFComm", "NFKernelPlugin", n + ".cpp")
            for n in ("NFCKernelModule", "NFCSceneAOIModule", "NFCEventModule", "NFCScheduleModule")] +
           [os.path.join(ref, "NFComm", "NFConfigPlugin", n + ".cpp") for n in ("NFCClassModule", "NFCElementModule")])
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-I", ref, "-I", os.path.join(ref, "Dependencies"),
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "resource_calls_ref.cpp"), *src, "-lpthread"], check=True)
    return exe


def main():
    ref = os.environ.get("REF", "/root/reference")
    exe = build(ref)
    script = rcm.golden_script()
    with tempfile.TemporaryDirectory() as d:
        sp = os.path.join(d, "script.txt")
        with open(sp, "w") as f:
            f.write("\n".join(script) + "\n")
        run = subprocess.run([exe, sp], capture_output=True, text=True, check=True)
    answers = []
    for ln in run.stdout.splitlines():
        if ln.startswith("A "):
            head, lst = ln.split(":")
            f = head.split()
            assert int(f[1]) == len(answers), ln
            answers.append([int(f[2]), [int(x) for x in lst.split()]])
    n = rcm.check_conditions(script, answers)
    dst = os.path.join(ROOT, "tests", "golden", "resource_calls.json")
    with open(dst, "w") as f:
        json.dump({"script": script, "props": rcm.PROPS, "answers": answers}, f, separators=(",", ":"))
    print(f"{dst}: {len(script)} lines, {len(answers)} answers, {os.path.getsize(dst)} bytes; conditions {n}")


if __name__ == "__main__":
    main()
