"""The yardstick of tests/test_gpu_bigsampler_subst.py, on the CPU: the C host driver on the REAL reference's locus API with the
three substitution-parameter moves on (alone, and with HRDT, MUI and MUBAR: a00_iterate's whole tail), on loci of the big-tree
sampler's kind — the 17-tip GTR sets, the forced 8-tip set, 24 tips whose scale counters fire — leaves a state that is its CPU
recompute at the current parameters; and the widths and the alpha prior the GPU firing test uses keep the oracle's counters
firing on the reference driver's chain alone."""
import numpy as np
import pytest

import firing
import heredity as HD
import hostdrv
import invariants
import locusrates as LR
import oraclelib as O
from test_gpu_bigsampler_subst import ALPHA0, configure_firing, param_firing, set17

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
ITERS = 20


def moved_on_host(drv, data):
    f = [i for i, d in enumerate(data) if list(drv.get_subst_model(i)[0]) != [float(x) for x in d["freqs"]]]
    q = [i for i, d in enumerate(data) if list(drv.get_subst_model(i)[1]) != [float(x) for x in d["exch"]]]
    a = [i for i in range(len(data)) if drv.get_subst_model(i)[2] != ALPHA0]
    return f, q, a


@needs_ref
@pytest.mark.parametrize("name,moves,tail", [("17-g4", "uniform", False), ("17-g4", "program", False), ("17-g4", "uniform", True),
                                             ("17-g4", "program", True), ("forced-8-gtr", "program", False),
                                             ("17-g1", "uniform", False), ("17-g1", "program", False)])
def test_host_driver_state_with_the_subst_moves(name, moves, tail):
    """20 iterations with the GPU trajectory test's sets and settings; every locus's lnl the oracle's at (tree, parameters,
    lengths x mu_i) to 1e-10, its density the one-locus driver's (at h_i) to 1e-11, tree shape, populations and buffer indices
    sound; every move was proposed, some proposals were accepted and every component moved (one category: alpha stays)"""
    c = dict(LR.case("b", 12), scaling=False) if name == "forced-8-gtr" else set17(1 if name == "17-g1" else 4)
    data, n = c["data"], len(c["data"])
    drv = HD.reference_driver(data, seed=31)
    if tail:
        HD.configure(drv, c, moves, True, subst=True, rates=True, scalars=HD.start_scalars(n))
    else:
        LR.configure(drv, c, moves, True, subst=True, ft=None)
    drv.initialize()
    p0 = drv.counters()[0]
    if tail:
        check = lambda: HD.check_state(drv, data, c["stree"][0], rated=True, tip_species=c["species"], subst=True)
    else:
        check = lambda: invariants.check_state(drv, data, c["stree"][0], tip_species=c["species"], subst=True)
    check()
    for _ in range(ITERS):
        drv.iterate()
    seen = check()
    p, a, _ = drv.counters()
    f, q, al = moved_on_host(drv, data)
    print(f"{name} {moves} tail {tail}: {seen}; accepted {a} of {p}; moved {f} / {q} / {al}")
    assert p - p0 > ITERS*(8 if name == "17-g1" else 9)*n and 0 < a < p
    assert len(f) == n and len(q) == n and (not al if name == "17-g1" else len(al) == n)
    if tail:
        hp, ha = drv.heredity_counters()
        cnt = drv.locusrate_counters()
        assert hp == ITERS*n and 0 < ha < hp and cnt["mui"][0] == ITERS*n and 0 < cnt["mui"][1] and cnt["mubar"][0] == ITERS
    drv.close()


@needs_ref
@pytest.mark.parametrize("moves", ["uniform", "program"])
def test_the_firing_set_keeps_firing_under_the_subst_moves(moves):
    """firing.case("big-24-gtr-g4") with the GPU firing test's widths and alpha prior on the reference-API driver, scaling on:
    fires_at_start at the starting parameters, still_fires at the chain's own trees and parameters after every one of 20
    iterations — the GPU test's input stays inside its own condition on the reference alone —, and the state is its CPU
    recompute with scale buffers"""
    c = firing.case("big-24-gtr-g4")
    data, n = c["data"], len(c["data"])
    with param_firing(data, [(d["freqs"], d["exch"], ALPHA0) for d in data]) as tagged:
        firing.fires_at_start(tagged)
        line = [firing.summary(tagged)]
    drv = hostdrv.reference_driver(data, seed=31, scaling=True)
    configure_firing(drv, c, moves, True)
    drv.initialize()
    for it in range(ITERS):
        drv.iterate()
        trees = [drv.tree(i) for i in range(n)]
        with param_firing(data, [drv.get_subst_model(i) for i in range(n)]) as tagged:
            firing.still_fires(tagged, trees)
            line.append(firing.summary(tagged, trees))
    seen = invariants.check_state(drv, data, c["stree"][0], tip_species=c["species"], scaling=True, subst=True)
    p, a, _ = drv.counters()
    f, q, al = moved_on_host(drv, data)
    print(f"big-24-gtr-g4 {moves}: nodes with a counter per locus / largest counter, start and after each iteration: "
          + "; ".join(f"{[x[0] for x in v]} / {max(x[1] for x in v)}" for v in line) + f"; {seen}; accepted {a} of {p}; moved {f} / {q} / {al}")
    assert 0 < a < p and len(f) == n and len(q) == n and len(al) == n
    drv.close()
