"""The program's THETA / TAU / MIX decisions of the persistent kernel where their lanes part ways: lgamma of a fit's shape a
is the library's below 16 (a call of the control wave's: sweep2.hpp, prog_lgamma_small), Stirling's series from 16 on, and a
lane without a population carries NaN through the series.  Loci counts at which the shapes fall on both sides of 16, against
the C host driver on the same seed."""
import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import hostdrv
import tape

pytestmark = pytest.mark.gpu

# (taxa, loci).  The shapes over the run's ten iterations, from the host driver (THETA's, TAU's and MIX's fits; priors 3 / 2,
# 300 sites, one sequence per species: populations 0 .. taxa - 1 have no theta and are NaN lanes in every decision, as is
# every lane but the step's three in a TAU decision):
#   4 taxa,  3 loci: all three inner populations below 16 (5.6 - 16.0): the library's lgamma and NaN lanes
#   4 taxa,  6 loci: populations 4, 5 below 16 (5.0 - 15.9, one fit of 16.7), the root 6 from 16 on (18 - 24; p = 0.3: 14.2 - 22.5) — THETA, MIX
#                    and the root's TAU (populations 6, 5 and the tip 3) hold all three kinds of lane at once
#   4 taxa, 24 loci: all from 16 on (23 - 50): the series and NaN lanes
#   8 taxa,  3 loci: all seven inner populations below 16 (5.6 - 14.2)
#   8 taxa,  9 loci: populations 10, 13 and the root 14 from 16 on (16 - 28), 8, 9, 11 below (8.7 - 16.7, a few draws above),
#                    12 on both sides (5.8 - 17.6) — all three kinds at once in THETA, MIX and the TAUs of 10, 13, 14
CASES = [(4, 3), (4, 6), (4, 24), (8, 3), (8, 9)]


@pytest.mark.parametrize("slide_prob", [0.0, 0.3])
@pytest.mark.parametrize("taxa,nloci", CASES)
def test_decisions_with_shapes_on_both_sides_of_16(taxa, nloci, slide_prob):
    """BPP's kernel and the program's moves, 10 iterations as three launches of one and a launch of seven: after every call
    the host driver's proposal / acceptance counts and Gibbs counters; at the end its taus, thetas and every locus's tree"""
    eng = bpp_amd.Engine(0)
    data = synth.make_dataset(nloci, 300, taxa, "jc69", 1, seed=100 + nloci)
    host = hostdrv.hip_driver(eng, tape.make_engine_loci(eng, data), data, seed=5)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=5)
    parent, tau0, thetas = synth.species_tree_arrays(taxa)
    for drv in (host, dev):
        drv.set_proposal_kernel(1)
        drv.set_program_moves(True, slide_prob)
        drv.set_species_tree(parent, tau0, thetas)
        drv.set_tau_prior(3.0, 3.0 / tau0[-1])
        drv.set_theta_prior(2.0, 1000.0, 0.0004)
        drv.set_finetune(0.003, 0.004, 0.0004, 0.1)
    host.initialize(); dev.initialize()
    assert dev.kind() == "persistent"
    for chunk in (1, 1, 1, 7):
        for _ in range(chunk):
            host.iterate()
        dev.iterate(chunk)
        s = dev.summary(); hp, ha, _ = host.counters()
        assert (s["proposals"], s["accepted"]) == (hp, ha), chunk
        assert dev.gibbs_counters() == host.gibbs_counters(), chunk
    assert np.allclose(dev.taus(), host.taus(), rtol=1e-10, atol=0) and np.allclose(dev.thetas(), host.thetas(), rtol=1e-10, atol=0)
    for i in range(nloci):
        a, b = dev.tree(i), host.tree(i)
        assert [int(x) for x in a["parent"]] == [int(x) for x in b["parent"]] and np.allclose(a["time"], b["time"], rtol=1e-10, atol=0), i
    host.close(); dev.close(); eng.close()
