"""Regenerate the `churn` golden fixture: tests/churn_worlds.py's tiny_groups world (160 objects in 16
small scene groups; every window creates and destroys 5 % of them and switches a quarter, into new groups
too, so scene groups drain to nobody and are joined again; records with SetRecordInt and row calls) run
through the REFERENCE's own classes (oracle/_ref/nf_ref_harness, built from the reference's sources by
oracle/build_ref.sh).  A machine without the reference pins the device on it through this fixture.

    python tests/golden/gen_churn_golden.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from noahgameframe_amd import nfio  # noqa: E402
from tests import churn_worlds  # noqa: E402


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "nf_ref_harness")
    w = churn_worlds.world(churn_worlds.GOLDEN_WORLD, churn_worlds.GOLDEN_TICKS)
    wp = os.path.join(HERE, "churn.workload.nfio")
    ep = os.path.join(HERE, "churn.expected.nfio")
    nfio.write(wp, w)
    subprocess.run([exe, wp, ep], check=True)
    print("churn", os.path.getsize(wp), os.path.getsize(ep))


if __name__ == "__main__":
    main()
