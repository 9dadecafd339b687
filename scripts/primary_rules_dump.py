"""The primary-marking workload (tests/primary_gen.py) and the reference's records for it (tests/golden/primary_golden.npz) as one binary file, for
scripts/primary_rules_main.cpp:   python scripts/primary_rules_dump.py OUT"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]
import numpy as np

import primary_gen as PG


def main(out):
    W, G = PG.workload(), PG.golden()
    n = W["reg_off"].shape[0] - 1
    head = np.array([n, W["regs"].shape[0], PG.ID_BASE, W["status_read"]], np.int64)
    with open(out, "wb") as f:
        for a, t in ((head, np.int64), (W["reg_off"], np.int64), (W["regs"], None), (G["regs"], None), (G["n_pri"], np.int32), (G["mapq"], np.uint8)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())


if __name__ == "__main__":
    main(sys.argv[1])
