"""The shaped sets of tests/shapes.py (loci at the device samplers' pattern- and tip-count limits) under the C host driver on
the REAL reference's locus API: the chain moves and accepts a sane share of its proposals on every set, with the priors and
step lengths the GPU tests give it — the acceptance band of invariants.moved is a condition on the DATA, checked here
before a GPU sees them.  GPU twin: tests/test_gpu_sampler_limits.py."""
import pytest

import oraclelib as O
import hostdrv
import shapes
from invariants import moved, check_state

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


def test_the_lists_reach_the_packing_s_edges():
    """no reference needed, but it belongs with the sets: the host-side packing of the two pattern-count lists"""
    shapes.check_lists()


def run(name, moves, iters, scaling=False):
    c = shapes.case(name)
    drv = hostdrv.reference_driver(c["data"], seed=7, scaling=scaling)
    shapes.configure(drv, c, moves, host=True)
    drv.initialize()
    for _ in range(iters):
        drv.iterate()
    p, a, _ = drv.counters()
    print(f"[limits] {name} {moves}: accepted {a / p:.3f} of {p}")
    moved(drv, c["stree"][1], c["stree"][2], p, a)
    return c, drv


# (loci of several kinds run the library's own proposal kernel only: the composite set has no 'program' case on the device)
@pytest.mark.parametrize("name,moves", [(n, m) for n in shapes.SMALL for m in ("uniform", "program") if (n, m) != ("composite-64-65", "program")])
def test_the_chain_moves_on_the_shaped_sets(name, moves):
    c, drv = run(name, moves, 30)
    if name == "persistent-mixed-tips":
        S = (len(c["stree"][0]) + 1) // 2
        assert all(a != b for a, b in zip(drv.thetas()[:S], c["stree"][2][:S])), "the tip populations' thetas never moved"
    drv.close()


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("moves", ["uniform", "program"])
@pytest.mark.parametrize("name", shapes.BIG)
def test_the_chain_moves_on_the_big_tree_sets(name, moves, scaling):
    c, drv = run(name, moves, 5, scaling)
    if name == "big-64-30" and moves == "uniform":
        # and the held state is the recompute's at 64 tips (the checker itself at the size the GPU test runs it at)
        check_state(drv, c["data"], c["stree"][0], tip_species=c["species"], scaling=scaling)
    drv.close()
