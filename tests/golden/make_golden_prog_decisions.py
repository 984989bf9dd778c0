"""What the program's THETA / TAU / MIX decide on the host, recorded BEFORE the host driver's statements of them
(csrc/host/a00_driver.c) and the generic sampler's (csrc/gsampler_host.hpp, host_decisions) became one (include/bpp_amd_priors.h:
a00_prog_*): the fixtures of tests/test_prog_decisions_host.py and tests/test_gpu_prog_decisions_sampler.py, whose cases and
readers these are.

    python tests/golden/make_golden_prog_decisions.py host    [commit [output]]   ->  tests/golden/prog_decisions_host.json, .npz
    python tests/golden/make_golden_prog_decisions.py sampler [commit [output]]   ->  tests/golden/prog_decisions_sampler.json, .npz

The .json holds the integers of every case, the .npz its doubles as they are (one array per case, under the case's name).

Run at the commit before the move (`commit`: its hash, kept in the fixture); `sampler` on the MI355X.  Every case runs twice,
each time on a fresh driver / engine: everything — integers and every float — must agree, or the generator stops: neither
fixture has holes.  The host driver's rows for 1 and for 4 threads must be equal too and are stored once."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def host(out, commit):
    import test_prog_decisions_host as T
    cases, floats = {}, {}
    for c in T.CASES:
        (i1, r1), (i2, r2) = T.run_case(*c), T.run_case(*c)
        assert i1 == i2, T.case_id(*c)
        T.same_bits(r1, r2)
        assert cases.setdefault(T.row_id(*c), i1) == i1, ("the thread count changed the counters", T.case_id(*c))
        T.same_bits(r1, floats.setdefault(T.row_id(*c), r1))                 # ... or the trajectory
        print(T.case_id(*c), i1, flush=True)
    return out or T.GOLDEN, cases, floats


def sampler(out, commit):
    import test_gpu_prog_decisions_sampler as T
    cases, floats = {}, {}
    for c in T.CASES:
        (i1, f1), (i2, f2) = T.run_case(*c), T.run_case(*c)
        assert i1 == i2, (T.case_id(*c), i1, i2)
        T.same_bits(f1, f2)
        cases[T.case_id(*c)], floats[T.case_id(*c)] = i1, f1
        print(T.case_id(*c), i1, flush=True)
    return out or T.GOLDEN, cases, floats


if __name__ == "__main__":
    what, commit, out = (sys.argv[1:] + [None, None, None])[:3]
    out, cases, floats = dict(host=host, sampler=sampler)[what](out, commit)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:                          # (a case a line)
        f.write('{"recorded_at": %s,\n "cases": {\n' % json.dumps(commit))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(cases[k], sort_keys=True)) for k in sorted(cases)))
        f.write("\n }}\n")
    np.savez_compressed(out[:-5] + ".npz", **floats)
