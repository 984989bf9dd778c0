"""How far the last places of libm move a discrete-gamma category rate: the bar of the device's rates (csrc/gamma_dev.hpp on
device exp / log / pow) against the host's (bpa_compute_gamma_cats on glibc), measured on the algorithm, not on a device.

    python tests/golden/make_golden_gamma_dev.py         ->  tests/golden/gamma_dev_sensitivity.json   (seconds)

csrc/gamma_dev.hpp is compiled as host code (tests/gammadev.py) with every exp / log / pow result moved by -1 / 0 / +1 ulp in a
seeded pseudo-random direction.  For every point of the grid (31 shapes alpha x 2 / 4 / 8 categories: every start-value branch of
chi2_quantile, the Wilson-Hilferty correction, both forms of incomplete_gamma) 200 such draws are evaluated and the largest
relative departure of any rate from the unperturbed value is recorded.  tests/test_gpu_subst_edges.py allows a device rate
gammadev.FACTOR (8) times that.

No recorded spread may exceed gammadev.SPREAD_CAP (1e-10): a draw that flips a series' termination test (accurate = 1e-8) would
show as ~1e-8, and a bar that wide would hide a truncated series.  The generator refuses to write such a point (it would have
to be replaced by a neighbour, and that said here); none of the grid's points needed replacing.
"""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gammadev                    # noqa: E402


def main():
    points = []
    with tempfile.TemporaryDirectory() as td:
        plain, pert = gammadev.build(td), gammadev.build(td, perturb=True)
        for K in gammadev.CATS:
            for alpha in gammadev.GRID:
                base = gammadev.gamma_cats(plain, alpha, K)
                assert np.isfinite(base).all() and (base > 0).all(), (alpha, K, base)
                s = pert.gd_spread(float(alpha), K, base.ctypes.data_as(C.POINTER(C.c_double)), gammadev.DRAWS, gammadev.SEED)
                assert 0 < s <= gammadev.SPREAD_CAP, f"alpha {alpha}, {K} categories: spread {s:.3e}"
                points.append(dict(alpha=float(alpha), cats=K, spread=s, smallest_rate=float(base[0])))
    out = dict(draws=gammadev.DRAWS, seed=gammadev.SEED, factor=gammadev.FACTOR, spread_cap=gammadev.SPREAD_CAP, points=points)
    with open(gammadev.FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for K in gammadev.CATS:
        sp = {p["alpha"]: p["spread"] for p in points if p["cats"] == K}
        print(f"{K} categories: " + "  ".join(f"{a:g}:{s:.1e}" for a, s in sp.items()))


if __name__ == "__main__":
    main()
