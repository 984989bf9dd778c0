"""The summation order of a sample-trace row's lnL on the host (plain helper module, no fixtures): csrc/kernels.hpp
trace_row_kernel adds the loci's lnl in lnl_sum_kernel's order, which include/bpp_amd.h documents — thread t of `threads`
adds values t, t + threads, ... in turn starting from 0.0, then the tree sh[t] += sh[t + w] for t < w, w = threads/2 ... 1."""
import numpy as np


def replay_sum(values, threads=1024):
    v = np.asarray(values, dtype=np.float64)
    assert threads >= 1 and threads & (threads - 1) == 0
    sh = np.zeros(threads)
    for t in range(min(threads, len(v))):
        acc = np.float64(0.0)
        for x in v[t::threads]:
            acc = acc + x
        sh[t] = acc
    w = threads // 2
    while w > 0:
        sh[:w] = sh[:w] + sh[w:2 * w]
        w //= 2
    return float(sh[0])


def replay_parts(parts, threads=1024):
    """a composite's row: every part's sum, added in part order"""
    tot = None
    for p in parts:
        x = np.float64(replay_sum(p, threads))
        tot = x if tot is None else tot + x
    return float(tot)


def any_order_bound(values):
    """n 2^-53 sum|x_i|: the rounding-error bound of a sum of n doubles, which holds for every order of the additions (Higham,
    Accuracy and Stability of Numerical Algorithms, section 4.2) — derived, not measured"""
    v = np.asarray(values, dtype=np.float64)
    return len(v) * 2.0 ** -53 * float(np.abs(v).sum())
