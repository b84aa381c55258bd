"""Generate tests/golden/dec_reject_matrix.json: what the built library answers to every case of
tests/dec_reject_cases.py (return code and stif_last_error() text per entry point and defect set).

The file pins the rejections of the decoder's entry points -- code, exact text, and which defect is reported when a
call has two -- so it is generated BEFORE a change to their host code and committed unchanged with it.  Every case is
a rejection (asserted), so no GPU is needed and no pointer is touched.  Run by hand:

    python tests/golden/make_dec_reject_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dec_reject_cases as R  # noqa: E402
import stif_pkg  # noqa: E402


def main():
    m = R.record(stif_pkg.load()._lib)
    with open(os.path.join(HERE, "dec_reject_matrix.json"), "w") as f:
        json.dump(m, f, indent=0)     # cases stay in list order
        f.write("\n")
    print(sum(len(e) for e in m["entries"].values()), "cases,", len(m["messages"]), "distinct answers")


if __name__ == "__main__":
    main()
