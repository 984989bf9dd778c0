"""csrc/gamma_dev.hpp (the device's discrete-gamma routine, gsampler.hpp: write_par) compiled as HOST code: `__device__`
defined away, g++ -O2 -ffp-contract=off, behind a C entry point (plain helper module, no fixtures).

Two builds of the same text:
  build(dir)                 the routine as it stands, on glibc's exp / log / pow: what tests/test_gamma_dev_host.py compares ==
                             with bpa_compute_gamma_cats (csrc/host_math.cpp, pinned to the reference)
  build(dir, perturb=True)   every exp / log / pow result moved by -1 / 0 / +1 ulp in a seeded pseudo-random direction: how far the
                             last places of libm move a rate.  tests/golden/make_golden_gamma_dev.py records that per grid point
                             (tests/golden/gamma_dev_sensitivity.json); the GPU test's bar is FACTOR x the recorded spread.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bpp_amd", "csrc", "gamma_dev.hpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gamma_dev_sensitivity.json")

# straddles 2 alpha = .32 and the -1.24 log p thresholds of chi2_quantile's start values for the quantiles of 2, 4 and 8 categories
GRID = (0.005, 0.01, 0.02, 0.05, 0.08, 0.1, 0.15, 0.159, 0.161, 0.17, 0.178, 0.18, 0.2, 0.3, 0.35, 0.36, 0.43, 0.5, 0.7, 0.86,
        1, 1.5, 2, 3, 5, 10, 20, 50, 100, 200, 500)
CATS = (2, 4, 8)
DRAWS, SEED = 200, 20240611
# the bar of a device rate at a grid point = FACTOR x the recorded spread: device exp / log may be off by 3 ulp where the draws
# move them by 1 (pow only feeds a start value the Newton steps forget) -> 4; 200 random sign patterns under-sample the worst
# alignment -> another 2
FACTOR = 8.0
# no recorded spread may exceed this: a flipped `term > accurate` / `dif <= accurate` (accurate = 1e-8) decision, which the bar
# must not hide, would show as ~1e-8
SPREAD_CAP = 1e-10

SHIM = r"""
#include <math.h>
#include <stdint.h>
#define __device__
#ifdef GD_PERTURB
namespace gdev {
static uint64_t gd_state = 1;
static inline double nudge(double x)
{
  gd_state ^= gd_state << 13; gd_state ^= gd_state >> 7; gd_state ^= gd_state << 17;         // xorshift64
  const int d = (int)((gd_state >> 11) % 3) - 1;
  if (!d || !isfinite(x) || x == 0) return x;
  return nextafter(x, d < 0 ? -INFINITY : INFINITY);
}
static inline double exp(double x) { return nudge(::exp(x)); }
static inline double log(double x) { return nudge(::log(x)); }
static inline double pow(double x, double y) { return nudge(::pow(x, y)); }
}
#endif
#include "gamma_dev.hpp"

extern "C" void gd_gamma_cats(double alpha, unsigned categories, double * rates) { gdev::gamma_cats(alpha, categories, rates); }

#ifdef GD_PERTURB
// largest relative departure of any rate from base[] over `draws` perturbed evaluations
extern "C" double gd_spread(double alpha, unsigned categories, const double * base, unsigned draws, uint64_t seed)
{
  double worst = 0, r[8];
  for (unsigned n = 0; n < draws; ++n)
  {
    gdev::gd_state = (seed + n)*0x9E3779B97F4A7C15ull | 1ull;
    gdev::gamma_cats(alpha, categories, r);
    for (unsigned k = 0; k < categories; ++k)
    {
      const double e = fabs(r[k] - base[k])/fabs(base[k]);
      if (!(e <= worst)) worst = e;                                                          // (a NaN sticks)
    }
  }
  return worst;
}
#endif
"""


def build(directory, perturb=False):
    """compile the shim around csrc/gamma_dev.hpp into `directory`; returns the ctypes library"""
    name = "gd_perturb" if perturb else "gd_plain"
    src, so = os.path.join(directory, name + ".cpp"), os.path.join(directory, "lib" + name + ".so")
    with open(src, "w") as f:
        f.write(SHIM)
    cmd = ["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.dirname(HEADER)] + \
          (["-DGD_PERTURB"] if perturb else []) + [src, "-o", so]
    subprocess.run(cmd, check=True)
    L = C.CDLL(so)
    L.gd_gamma_cats.restype, L.gd_gamma_cats.argtypes = None, [C.c_double, C.c_uint, C.POINTER(C.c_double)]
    if perturb:
        L.gd_spread.restype = C.c_double
        L.gd_spread.argtypes = [C.c_double, C.c_uint, C.POINTER(C.c_double), C.c_uint, C.c_uint64]
    return L


def gamma_cats(L, alpha, cats):
    out = np.zeros(cats)
    L.gd_gamma_cats(float(alpha), int(cats), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def load_bars():
    """{cats: (log alpha of the grid points, FACTOR x recorded spread)} from the committed fixture"""
    with open(FIXTURE) as f:
        g = json.load(f)
    bars = {}
    for K in CATS:
        pts = sorted((p["alpha"], p["spread"]) for p in g["points"] if p["cats"] == K)
        bars[K] = (np.log([a for a, _ in pts]), FACTOR * np.array([s for _, s in pts]))
    return bars


def bar(bars, alpha, cats):
    """the bar of the grid point nearest to alpha (in log alpha)"""
    la, b = bars[cats]
    return float(b[int(np.argmin(np.abs(la - np.log(alpha))))])
