"""The record-finishing workload (tests/finish_gen.py) and the reference's records for it (tests/golden/finish_golden.npz) as one binary file, for
scripts/finish_rules_main.cpp:   python scripts/finish_rules_dump.py OUT"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]
import numpy as np

import finish_gen as FG


def main(out):
    W = FG.workload()
    want, want_off, want_ums = FG.golden()
    want = FG.take(want, np.arange(want.shape[0]))
    n = W["reg_off"].shape[0] - 1
    alt = np.array([c[2] for c in W["contigs"]], np.uint8)
    head = np.array([n, W["regs"].shape[0], W["reads"].shape[0], W["text"].shape[0], W["l_pac"], alt.shape[0], want.shape[0], 0], np.int64)
    with open(out, "wb") as f:
        for a, t in ((head, np.int64), (W["reg_off"], np.int64), (W["read_off"], np.int64), (W["regs"], None), (W["reads"], np.uint8), (W["text"], np.uint8), (alt, np.uint8),
                     (want_off, np.int64), (want_ums, np.uint8), (want, None)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())


if __name__ == "__main__":
    main(sys.argv[1])
