"""The device's discrete-gamma routine (csrc/gamma_dev.hpp: what the generic sampler's alpha move runs for every proposal and
every rejected one) pinned WITHOUT a GPU: its text compiled as host code (tests/gammadev.py: `__device__` defined away, g++ -O2
-ffp-contract=off) gives the rates of bpa_compute_gamma_cats (csrc/host_math.cpp) to the bit — which tests/test_abi.py and
tests/test_oracle_pin.py pin bit-exact to the reference.  On the same libm the two copies of the published routines must not
differ at all: the day one of them is edited and the other is not, this fails.  On the device the same text runs on another
libm; how far that may move a rate is tests/golden/gamma_dev_sensitivity.json (tests/golden/make_golden_gamma_dev.py), the bar of
tests/test_gpu_subst_edges.py.
"""
import numpy as np
import pytest

import bpp_amd
import gammadev


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return gammadev.build(str(tmp_path_factory.mktemp("gamma_dev")))


def same(L, alpha, K):
    want = bpp_amd.compute_gamma_cats(alpha, alpha, K)
    got = gammadev.gamma_cats(L, alpha, K)
    assert np.isfinite(want).all() and (want > 0).all(), (alpha, K, want)
    assert (got == want).all(), (alpha, K, [x.hex() for x in got], [x.hex() for x in want])
    return want


def test_grid_is_bit_identical_to_the_host_routine(plain):
    """every start-value branch of chi2_quantile (v < -1.24 log p; v > .32, with and without the Wilson-Hilferty correction;
    the small-v Newton loop) and both forms of incomplete_gamma"""
    small = None
    for K in range(2, 9):
        for alpha in gammadev.GRID:
            r = same(plain, alpha, K)
            assert (np.diff(r) > 0).all(), (alpha, K, r)
            if K == 8 and alpha == 0.005:
                small = r[0]
    assert 1e-182 < small < 2e-181          # the smallest rate of the grid is a normal number


def test_random_sweep_is_bit_identical_to_the_host_routine(plain):
    rng = np.random.default_rng(20240611)
    n = 4000
    alphas = np.exp(rng.uniform(np.log(0.005), np.log(500.0), n))
    cats = rng.integers(2, 9, n)
    for alpha, K in zip(alphas, cats):
        same(plain, float(alpha), int(K))
    # one category: the rate is 1 (both copies short-cut it)
    assert gammadev.gamma_cats(plain, 0.7, 1)[0] == 1.0 == bpp_amd.compute_gamma_cats(0.7, 0.7, 1)[0]


def test_the_committed_sensitivity_covers_the_grid_within_its_cap():
    """the fixture the GPU bars come from: one record per (grid alpha, 2 / 4 / 8 categories), each spread measured (> 0) and
    below the cap that keeps a bar from hiding a truncated series (accurate = 1e-8)"""
    import json
    with open(gammadev.FIXTURE) as f:
        g = json.load(f)
    assert (g["draws"], g["seed"], g["factor"], g["spread_cap"]) == (gammadev.DRAWS, gammadev.SEED, gammadev.FACTOR, gammadev.SPREAD_CAP)
    assert sorted((p["cats"], p["alpha"]) for p in g["points"]) == sorted((K, float(a)) for K in gammadev.CATS for a in gammadev.GRID)
    assert all(0 < p["spread"] <= gammadev.SPREAD_CAP for p in g["points"])
    bars = gammadev.load_bars()
    assert gammadev.bar(bars, 0.5, 4) == gammadev.FACTOR * next(p["spread"] for p in g["points"] if (p["cats"], p["alpha"]) == (4, 0.5))
    assert gammadev.bar(bars, 0.1604, 8) == gammadev.bar(bars, 0.161, 8) and gammadev.bar(bars, 700.0, 2) == gammadev.bar(bars, 500.0, 2)
