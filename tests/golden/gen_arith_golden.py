"""Regenerate the `arith` golden fixture: tests/arith_edges.py's combined world (float_props' float ops
with non-dyadic constants, float_consts' compiler-foldable constants and int_edges' int64 extremes over
NaN / inf / +-DBL_MAX / threshold-sized / -0.0 / denormal values; properties only — the reference's own
NFCRecord::SetFloat is broken, so the record edges are pinned on the oracle) run through the REFERENCE's
own classes (oracle/_ref/nf_ref_harness, built from the reference's sources by oracle/build_ref.sh).

    python tests/golden/gen_arith_golden.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from noahgameframe_amd import nfio  # noqa: E402
from tests import arith_edges  # noqa: E402


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "nf_ref_harness")
    w = arith_edges.arith(arith_edges.ARITH_SEED)
    wp = os.path.join(HERE, "arith.workload.nfio")
    ep = os.path.join(HERE, "arith.expected.nfio")
    nfio.write(wp, w)
    subprocess.run([exe, wp, ep], check=True)
    print("arith", os.path.getsize(wp), os.path.getsize(ep))


if __name__ == "__main__":
    main()
