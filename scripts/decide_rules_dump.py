"""The pairing-decision workload as the stage takes it (tests/decide_cases.py: stage_inputs) and the model's results for it as one binary file, for
scripts/decide_rules_main.cpp:   python scripts/decide_rules_dump.py OUT"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "bwa-meme_amd")]

import decide_cases

if __name__ == "__main__":
    decide_cases.dump(sys.argv[1])
