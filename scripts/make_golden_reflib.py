"""Generate tests/golden/reflib_digests.json: what the UNMODIFIED reference C++ front end (oracle/_ref/libpcrcg_ref.so,
built by oracle/Makefile from the reference's cpp_wrappers.zip) returns on the fixed inputs of the reference-library tests
in tests/test_oracle_frontend.py, so that those tests compare the oracle against the reference without it.

Runs only where oracle/_ref is built.  The lattice cases are the 60 examples a derandomised hypothesis property test draws;
they are stored with the digests, so the test replays them without hypothesis.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import frontend as F  # noqa: E402
from tests import test_oracle_frontend as T  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "reflib_digests.json")


def lattice_cases():
    from hypothesis import given, settings, strategies as st
    cases = []

    @settings(max_examples=60, deadline=None, derandomize=True, database=None)
    @given(st.integers(1, 120), st.integers(1, 90), st.integers(2, 9), st.sampled_from([0.25, 0.5, 1.0, 1.7]),
           st.integers(0, 2 ** 31 - 1))
    def collect(n0, n1, lattice, dl, seed):
        if [n0, n1, lattice, dl, seed] not in cases:
            cases.append([n0, n1, lattice, dl, seed])

    collect()
    return cases


def main():
    if not F.have_ref():
        sys.exit("oracle/_ref/libpcrcg_ref.so is not built (make -C oracle ref where the reference is present)")
    cases = lattice_cases()
    out = {"library": T.library_records("ref"),
           "lattice": {"cases": cases, "records": T.lattice_records("ref", cases)},
           "tie_order": T.tie_order_records("ref")}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT, "(%d lattice cases, %d tie-order cases)" % (len(cases), len(out["tie_order"])))


if __name__ == "__main__":
    main()
