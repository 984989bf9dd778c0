"""The generic sampler's host_decisions form (csrc/gsampler_host.hpp: gs_prog_theta / _tau / _mix, gs_mubar's host branch) takes
the program's THETA / TAU / MIX decisions from the ONE statement of them in include/bpp_amd_priors.h (a00_prog_*), which the C
host driver calls too.  This test holds it to what its own copy of those statements did before they moved:
tests/golden/prog_decisions_sampler.json (the integers) and .npz (the doubles, as recorded: compared through their 64 bits) were
taken on the MI355X at the commit before the move (tests/golden/make_golden_prog_decisions.py sampler).  CPU twin, for the host
driver's side: tests/test_prog_decisions_host.py.  (tests/test_gpu_prog_decisions.py is about the DEVICE's decisions, which did
not move.)

Every case is a generic sampler with host_decisions=True and the program's moves, 6 iterations as iterate(1), iterate(2),
iterate(3); then summary() (launches, proposals, accepted), the Gibbs, rate and heredity counters — integers — and taus, thetas,
total lnL, rates, their mean and the scalars — bit for bit (a mismatch is shown as hex floats).  The generator ran every case
twice: nothing was unreproducible, nothing is left out.  The margin is zero because host code moved and nothing else.

Cases: {8-tip GTR+Gamma4, 60 sites, 6 loci; 4-species JC69, 8 loci} x theta / tau prior kind {gamma, inverse gamma} x slide_prob
{0, 0.1, 1} x heredity {off, scalars != 1 with the HRDT move} x {rates fixed at 1, rates with MUI and MUBAR: gs_mubar's host
branch}; and with the one-rank all-reduce callback `lambda p, n, st: 1`, which drives the split64 / join64 packing of the sums:
the library takes a callback with gamma priors, without rate moves and without the heredity move only (bpa_sampler_set_allreduce,
bpa_sampler_iterate refuse the rest), so those cases are gamma x slide_prob x heredity {off, fixed scalars != 1}."""
import json
import os

import numpy as np
import pytest

import bpp_amd
from bpp_amd import synth
import heredity as HD
import locusrates as LR
import tape
from test_prog_decisions_host import same_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prog_decisions_sampler.json")
SEED = 37
CALLS = (1, 2, 3)

# (shape, prior kind, slide_prob, heredity, MUI + MUBAR, all-reduce callback)
CASES = [(sh, k, sl, h, m, False) for sh in ("gtr8", "jc4") for k in ("gamma", "invgamma") for sl in (0.0, 0.1, 1.0) for h in (False, True) for m in (False, True)]
CASES += [(sh, "gamma", sl, h, False, True) for sh in ("gtr8", "jc4") for sl in (0.0, 0.1, 1.0) for h in (False, True)]


def case_id(shape, kind, slide, hered, mubar, callback):
    return f"{shape}-{kind}-slide{slide:g}-{'hered' if hered else 'nohered'}-{'mubar' if mubar else 'norates'}" + ("-callback" if callback else "")


_DATA = {}


def data_of(shape):
    """built once, never changed -> (data, stree)"""
    if shape not in _DATA:
        _DATA[shape] = (synth.make_dataset(6, 60, 8, "gtr", 4, seed=91), synth.species_tree_arrays(8)) if shape == "gtr8" else \
                       (synth.make_dataset(8, 60, 4, "jc69", 1, seed=92), synth.species_tree_arrays(4))
    return _DATA[shape]


FLOATS = ("taus", "thetas", "total_lnl", "rates", "mubar", "scalars")          # the order of a case's vector in the .npz


def run_case(shape, kind, slide, hered, mubar, callback):
    """-> (integers, the floats in the order of FLOATS as one vector) of the case after its 6 iterations"""
    data, (parent, tau0, thetas) = data_of(shape)
    n = len(data)
    eng = bpp_amd.Engine(0)
    dev = bpp_amd.Sampler(eng, tape.make_engine_loci(eng, data), data, seed=SEED, implementation="generic", host_decisions=True)
    dev.set_proposal_kernel(1)
    dev.set_program_moves(True, slide)
    dev.set_species_tree(parent, tau0, thetas)
    if kind == "invgamma":                 # means at the start values: b = (a - 1) x mean
        dev.set_tau_prior(3.0, 2.0*tau0[-1]); dev.set_theta_prior(3.0, 0.004, 0.001); dev.set_finetune(0.003, 0.005, 0.0008, 0.2)
        dev.set_prior_kinds("invgamma", "invgamma")
    else:
        dev.set_tau_prior(3.0, 3.0/tau0[-1]); dev.set_theta_prior(2.0, 1000.0, 0.0004); dev.set_finetune(0.003, 0.005, 0.0004, 0.05)
    if mubar:
        dev.set_locus_rates(LR.spread_rates(n, 0.5, 2.0))
        dev.set_locusrate_moves(0.5, 0.4, 5.0, 10.0, 10.0, 1.0)
    if hered:
        dev.set_heredity(HD.start_scalars(n))
        if not callback:
            dev.set_heredity_move(0.6, 4.0, 4.0)
    if callback:
        dev.set_allreduce(lambda p, n_, st: 1, 0, 0)
    dev.initialize()
    assert dev.kind() == "generic"
    for k in CALLS:
        dev.iterate(k)
    s = dev.summary()
    rates = dev.locusrate_counters()
    ints = dict(launches=s["launches"], proposals=s["proposals"], accepted=s["accepted"], gibbs=list(dev.gibbs_counters()),
                mui=list(rates["mui"]), mubar=list(rates["mubar"]), heredity=list(dev.heredity_counters()))
    mui, mean = dev.get_locus_rates()
    floats = dict(taus=dev.taus(), thetas=dev.thetas(), total_lnl=[s["total_lnl"]], rates=mui, mubar=[mean], scalars=dev.get_heredity())
    dev.close()
    eng.close()
    return ints, np.concatenate([np.asarray(floats[k], dtype=np.float64).ravel() for k in FLOATS])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    with np.load(GOLDEN[:-5] + ".npz") as z:
        g["floats"] = {k: z[k] for k in z.files}
    return g


def test_the_fixture_has_every_case(golden):
    assert set(golden["cases"]) == set(golden["floats"]) == {case_id(*c) for c in CASES}


@pytest.mark.parametrize("shape,kind,slide,hered,mubar,callback", CASES, ids=[case_id(*c) for c in CASES])
def test_sampler_decides_on_the_host_as_before_the_move(golden, shape, kind, slide, hered, mubar, callback):
    cid = case_id(shape, kind, slide, hered, mubar, callback)
    ints, floats = run_case(shape, kind, slide, hered, mubar, callback)
    nloci = len(data_of(shape)[0])
    print(f"[prog-decisions-sampler] {case_id(shape, kind, slide, hered, mubar, callback)}: {ints}")
    assert ints == golden["cases"][cid]
    assert ints["proposals"] > ints["accepted"] > 0
    npop_theta = (15 if shape == "gtr8" else 7) - (8 if shape == "gtr8" else 4)          # one sequence a species: the inner populations
    if slide in (0.0, 1.0):                # (at 0.1 the choices are the stream's: the fixture's integers hold them)
        assert ints["gibbs"][0] == (0 if slide == 1.0 else sum(CALLS)*npop_theta)
    if kind == "invgamma":
        assert ints["gibbs"][1] == ints["gibbs"][0]
    if mubar:
        assert ints["mui"][0] == sum(CALLS)*nloci and ints["mubar"][0] == sum(CALLS)
    if hered and not callback:
        assert ints["heredity"][0] == sum(CALLS)*nloci
    same_bits(floats, golden["floats"][cid])
