"""Records tests/golden/jump_exact_ill.json on the CPU: on every ill-conditioned s-grid of tests/jump_cases.py (the placements of
ill_grids.s_positions at m1 = 50 and 600, one interval 1e6 times shorter than its neighbour) and every law of jump_cases.ILL_LAWS,
the distance of the numpy generator (tests/jumps_ref.py, the formula of hadi_jump_entry_value) from the 40-digit generator of
tests/jumps_exact.py -- per checked row the largest entry distance and the distance of the sum of the two columns around the tiny
interval.  The emulator and device tests judge the device matrix by 30 times these (ill_grids.FACTOR) without needing mpmath;
tests/test_jumps_exact.py compares what it recomputes with the file.

    python tools/record_jump_exact.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FIXTURE = os.path.join(ROOT, "tests", "golden", "jump_exact_ill.json")


def main():
    import __graft_entry__ as G
    G.build_oracle()
    import jump_cases as JC
    import test_jumps_exact as TX
    cases = {}
    for m1, _ in JC.ILL_SHAPES:
        places, K = JC.ill_s_grids(m1)
        for name, vs, ds, tiny in places:
            rows = JC.ill_rows(m1, tiny)
            for law in JC.ILL_LAWS:
                dist, sums, _, _ = TX.ill_measure(vs, tiny, law, rows)
                cases[JC.ill_key(m1, name, law)] = {"tiny": tiny, "rows": rows, "dist": dist, "sum_dist": sums}
                print("%s: worst entry %.2e, worst sum %.2e" % (JC.ill_key(m1, name, law), max(dist), max(sums)), flush=True)
    with open(FIXTURE, "w") as f:
        json.dump({"R": JC.ILL_R, "digits": 40, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
