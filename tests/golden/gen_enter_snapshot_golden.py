"""Writes tests/golden/enter_snapshot.json: the reference's own enter payloads over
tests.enter_snapshot_model.golden_script().

Run by hand on a machine that has the reference tree (REF, default /root/reference); not part of the
build.  tests/cpp/enter_snapshot_ref.cpp is compiled against the reference's NFCPropertyManager /
NFCRecordManager (NFCProperty, NFCRecord, NFCDataList) sources where they lie into
oracle/_ref/enter_snapshot_ref and run on the script; only the script and its recorded answers are kept.

    python tests/golden/gen_enter_snapshot_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import enter_snapshot_model as esm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
CORE = ["NFCDataList", "NFCRecord", "NFCRecordManager", "NFCProperty", "NFCPropertyManager", "NFMemoryCounter"]


def parse(stdout):
    """the V / P / R lines of enter_snapshot_ref / enter_snapshot_plugin ->
    [[[name, bits(, head)] ...], [[rec, used, [cells]] ...]] per snapshot, in call order"""
    out = []
    for ln in stdout.splitlines():
        f = ln.split()
        if not f:
            continue
        if f[0] == "V":
            assert int(f[1]) == len(out), ln
            out.append([[], []])
            want = (int(f[2]), int(f[3]))
        elif f[0] == "P":
            out[-1][0].append([f[1]] + [int(x) for x in f[2:]])
        elif f[0] == "R":
            out[-1][1].append([f[1], int(f[2]), [int(x) for x in f[4:]]])
        if f[0] in "PR" and f[0] != "V":
            assert len(out[-1][0]) <= want[0] and len(out[-1][1]) <= want[1], ln
    return out


def _f(bits):
    return float(np.uint64(bits).view(np.float64))


def check_conditions(script, answers):
    """what the golden is there for (asserted again by tests/test_enter_snapshot.py)"""
    snaps = [ln.split() for ln in script if ln.startswith("S ")]
    assert len(snaps) == len(answers)
    props = {ln.split()[1]: (ln.split()[2], int(ln.split()[3])) for ln in script if ln.startswith("PROP ")}
    names = list(props)
    # names whose byte order differs from definition order: an upper-case name, "a10" < "a9"
    order = [names[i] for i in esm.name_order(names)]
    assert order != names and any(n[0].isupper() for n in names)
    assert order.index("a10") < order.index("a9") and order.index("Zeta") < order.index("alpha")
    both = [a for a in answers if {"a10", "a9"} <= {p[0] for p in a[0]}]
    assert both and all([p[0] for p in a[0]].index("a10") < [p[0] for p in a[0]].index("a9") for a in both)
    for a in answers:   # every walk is in byte-wise name order
        got = [p[0].encode() for p in a[0]]
        assert got == sorted(got)
        got = [r[0].encode() for r in a[1]]
        assert got == sorted(got)
    # flags: both, neither, upload only
    assert any(f == 3 for _, f in props.values()) and any(f == 0 for _, f in props.values())
    assert any(f == esm.UPLOAD for _, f in props.values())
    packed = {p[0] for a in answers for p in a[0]}
    assert "hidden" not in packed and "up" not in packed and "alpha" in packed
    for s, a in zip(snaps, answers):
        for p in a[0]:
            assert props[p[0]][1] & (esm.PRIVATE if s[2] == "1" else esm.PUBLIC)
    # the null boundary: every kept value is packed somewhere, no dropped one ever is
    fvals = {p[1] for a in answers for p in a[0] if props[p[0]][0] == "F"}
    for v in esm.F_KEPT:
        assert esm.f64_bits(v) in fvals, v
    for b in fvals:
        assert _f(b) > 0.001 or _f(b) < -0.001
    set_f = {ln.split()[3] for ln in script if ln.startswith("SF ")}
    for v in esm.F_DROPPED:
        assert float(v).hex() in set_f, v
    ivals = {p[1] for a in answers for p in a[0] if props[p[0]][0] == "I"}
    assert esm.i64_bits(-(1 << 63)) in ivals and (1 << 32) in ivals and 0 not in ivals
    ovals = [(p[1], p[2]) for a in answers for p in a[0] if props[p[0]][0] == "O"]
    assert any(d and not h for d, h in ovals) and any(h and not d for d, h in ovals) and (0, 0) not in ovals
    # a record in view with no used row; a record whose removed row still holds a value
    assert any(r[1] == 0 and r[2] == [] for a in answers for r in a[1])
    i = script.index("RM 1 bag 2")
    assert "AR 1 bag 2 11 0 0x1.8p+0" in script[:i]
    first = answers[[k for k, s in enumerate(snaps) if s[1] == "1" and s[2] == "0"][0]]
    bag = [r for r in first[1] if r[0] == "bag"][0]
    assert bag[1] == 1 and 11 not in bag[2] and len(bag[2]) == 3
    assert sum(1 for a in answers if a[0] or any(r[1] for r in a[1])) >= 30, "non-empty views"


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "enter_snapshot_ref")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(REF, "NFComm", "NFCore", n + ".cpp") for n in CORE]
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I", REF, "-I", os.path.join(REF, "Dependencies"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "enter_snapshot_ref.cpp"), *src, "-lpthread"], check=True)
    script = esm.golden_script()
    with tempfile.TemporaryDirectory() as d:
        sp = os.path.join(d, "script.txt")
        with open(sp, "w") as f:
            f.write("\n".join(script) + "\n")
        run = subprocess.run([exe, sp], capture_output=True, text=True, check=True)
    answers = parse(run.stdout)
    check_conditions(script, answers)
    path = os.path.join(ROOT, "tests", "golden", "enter_snapshot.json")
    with open(path, "w") as f:
        json.dump({"world": "tests.enter_snapshot_model.golden_script()", "script": script, "answers": answers}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(answers)} snapshots, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
