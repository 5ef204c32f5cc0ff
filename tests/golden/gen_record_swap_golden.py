"""Writes tests/golden/record_swap.json: the reference's own answers on NFCRecord::SwapRowInfo among the
other record calls, over tests.record_swap_model.golden_script().

Run by hand on a machine that has the reference tree (REF, default /root/reference); not part of the
build.  tests/cpp/record_swap_ref.cpp is compiled against the reference's NFCRecord and NFCDataList
sources where they lie into oracle/_ref/record_swap_ref and run on the script; only the script and
its recorded answers are kept.

    python tests/golden/gen_record_swap_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import record_object_model as rom  # noqa: E402
from tests import record_swap_model as rsm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
CORE = ["NFCDataList", "NFCRecord", "NFMemoryCounter"]


def parse(stdout):
    """the E / A lines of record_swap_ref / record_swap_plugin -> [[ret, list, events]] in call order"""
    out, ev = [], []
    for ln in stdout.splitlines():
        if ln.startswith("E "):
            f = ln.split()
            assert int(f[1]) == len(out), ln
            ev.append([int(x) for x in f[2:5]] + [rom.u64(int(x)) for x in f[5:9]])
        elif ln.startswith("A "):
            head, lst = ln.split(":")
            f = head.split()
            assert int(f[1]) == len(out), ln
            out.append([int(f[2]), [int(x) for x in lst.split()], ev])
            ev = []
    return out


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "record_swap_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(REF, "NFComm", "NFCore", n + ".cpp") for n in CORE]
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I", REF, "-I", os.path.join(REF, "Dependencies"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "record_swap_ref.cpp"), *src, "-lpthread"], check=True)
    script = rsm.golden_script()
    with tempfile.TemporaryDirectory() as d:
        sp = os.path.join(d, "script.txt")
        with open(sp, "w") as f:
            f.write("\n".join(script) + "\n")
        run = subprocess.run([exe, sp], capture_output=True, text=True, check=True)
    answers = parse(run.stdout)
    counts = rsm.check_conditions(script, answers)   # (the seed is chosen so that this holds)
    path = os.path.join(ROOT, "tests", "golden", "record_swap.json")
    with open(path, "w") as f:
        json.dump({"world": "tests.record_swap_model.golden_script()", "script": script, "answers": answers}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(answers)} calls, {os.path.getsize(path)} bytes")
    print(counts)


if __name__ == "__main__":
    main()
