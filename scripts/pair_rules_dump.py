"""The pair-scoring workload (tests/pair_gen.py) and the reference's outputs for it (tests/golden/pair_golden.npz) as one binary file, for
scripts/pair_rules_main.cpp:   python scripts/pair_rules_dump.py OUT"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]

import pair_cases

if __name__ == "__main__":
    pair_cases.dump(sys.argv[1])
