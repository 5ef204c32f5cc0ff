"""Writes tests/golden/record_find.json: the reference's own answers to the record finds over
tests.record_find_model.golden_script().

Run by hand on a machine that has the reference tree (REF, default /root/reference); not part of the
build.  tests/cpp/record_find_ref.cpp is compiled against the reference's NFCRecord and NFCDataList
sources where they lie into oracle/_ref/record_find_ref and run on the script; only the script and
its recorded answers are kept.

    python tests/golden/gen_record_find_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import record_find_model as rfm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
CORE = ["NFCDataList", "NFCRecord", "NFMemoryCounter"]


def parse(stdout):
    """the A lines of record_find_ref / record_find_plugin -> [[ret, list]] in call order"""
    out = []
    for ln in stdout.splitlines():
        if not ln.startswith("A "):
            continue
        head, lst = ln.split(":")
        f = head.split()
        assert int(f[1]) == len(out), ln
        out.append([int(f[2]), [int(x) for x in lst.split()]])
    return out


def check_conditions(script, answers):
    """what the golden is there for (asserted again by tests/test_record_find.py)"""
    calls = [ln for ln in script if ln[0] in "FQ"]
    assert len(calls) == len(answers)
    finds = [(c.split(), a) for c, a in zip(calls, answers) if c[0] == "F"]
    assert sum(1 for c, a in finds if a[1]) >= 30, "calls with a non-empty list"
    assert sum(1 for c, a in finds if len(a[1]) > 1) >= 5, "calls with more than one row"
    assert sum(1 for c, a in finds if a[0] == -1) >= 3, "calls returning -1"
    assert any(63 in a[1] for c, a in finds), "a find that hits row 63"
    # a re-added row holding 0: `AR o 0 5` (no values) directly followed by `FI o 0 0 0` that finds row 5
    hit = False
    for i, ln in enumerate(script[:-1]):
        f = ln.split()
        if f[0] == "AR" and len(f) == 4 and script[i + 1] == f"FI {f[1]} {f[2]} 0 0":
            k = sum(1 for x in script[:i + 1] if x[0] in "FQ")
            hit = hit or int(f[3]) in answers[k][1]
    assert hit, "a find that hits a re-added row holding 0"


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "record_find_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(REF, "NFComm", "NFCore", n + ".cpp") for n in CORE]
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I", REF, "-I", os.path.join(REF, "Dependencies"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "record_find_ref.cpp"), *src, "-lpthread"], check=True)
    script = rfm.golden_script()
    with tempfile.TemporaryDirectory() as d:
        sp = os.path.join(d, "script.txt")
        with open(sp, "w") as f:
            f.write("\n".join(script) + "\n")
        run = subprocess.run([exe, sp], capture_output=True, text=True, check=True)
    answers = parse(run.stdout)
    check_conditions(script, answers)
    path = os.path.join(ROOT, "tests", "golden", "record_find.json")
    with open(path, "w") as f:
        json.dump({"world": "tests.record_find_model.golden_script()", "script": script, "answers": answers}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(answers)} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
