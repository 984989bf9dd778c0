"""What the generic and the big-tree sampler compute and launch in 6 iterations, recorded BEFORE their two launch loops
became one (csrc/gsampler_host.hpp: gs_iterate): the fixture of tests/test_gpu_launch_loop.py, whose cases and reader these are.

    python tests/golden/make_golden_launch_loop.py [output [commit]]     ->  tests/golden/launch_loop.json

Run on the MI355X at the commit before the join (`commit`: its hash, kept in the fixture).  Every case runs twice, each time
on a fresh engine: the integers (launches, proposals, acceptances, the moves' counters) must agree, or the generator stops; a
float that differs between the two runs is left out of that case and named under its "unreproducible"."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_gpu_launch_loop import CASES, GOLDEN, case_id, run_case          # noqa: E402


def main(out, commit):
    cases = {}
    for c in CASES:
        (i1, f1), (i2, f2) = run_case(*c), run_case(*c)
        assert i1 == i2, (case_id(*c), i1, i2)
        keep = {k: v for k, v in f1.items() if f2[k] == v}
        cases[case_id(*c)] = dict(ints=i1, floats=keep, unreproducible=sorted(set(f1) - set(keep)))
        print(case_id(*c), i1, "unreproducible:", cases[case_id(*c)]["unreproducible"], flush=True)
    with open(out, "w") as f:
        json.dump(dict(recorded_at=commit, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, sys.argv[2] if len(sys.argv) > 2 else None)
