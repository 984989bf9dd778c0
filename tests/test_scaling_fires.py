"""The firing sets of tests/firing.py on the CPU: every set proves what it claims about its own scale counters (from the oracle),
and the C host driver over the REAL reference's locus API (hostdrv.reference_driver, scaling=True) keeps every invariant of
tests/invariants.py: check_state on them — at the start, at two checkpoints and at the end — while the counters go on firing.
This pins the data, the priors and the run lengths of the device tests (tests/test_gpu_scaling_fires.py) without a device.

How the sets were chosen (all measured here, with this driver; tests/firing.py says the same where each choice is made):
  * 8-tip 4-state loci never fire; three sequences per species fire below the root in some trees only — six such 24-tip loci had
    no firing node below any root at 3 of 48 checkpoints under JC69 and at 2 of 48 under GTR+Gamma4 (6 driver seeds x 2 kinds of
    moves x iterations 1, 3, 30, 60), and fewer loci lose it more often; with ten
    sequences of one species there were 3 .. 6 of 6 loci with one at every checkpoint up to 30 iterations, over the same seeds;
  * with tests/shapes.py's priors and steps x f the program's moves took tau to 25 x and theta to 50 x their start within 60
    iterations (random columns want long branches) and the 17-tip loci stopped firing; with firing_case's narrow priors and
    tenth-size steps: tau 1.2 - 1.3 x, theta 1.8 - 2.1 x after 30, acceptance 0.28 - 0.45 — inside invariants.moved()'s band;
  * 17 tips (JC69) and 16 tips (LG) fire once per path at any f >= 1e-6: a 24-tip locus beside them carries the counter of 2.
Each test prints the nodes with a counter per locus and checkpoint (pytest -rP).  Device runs: the table of
tests/test_gpu_state_invariants.py.
"""
import numpy as np
import pytest

import oraclelib as O
import hostdrv
import shapes
import firing
import tape
from invariants import check_state, moved

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")

SAMPLER_SETS = ["big-17", "big-24", "big-24-gtr-g4", "big-64"]
PLAN_SETS = ["plan-jc69-1-5", "plan-jc69-1-3", "plan-gtr-1-5", "plan-gtr-1-3", "plan-gtr-3-5", "plan-gtr-3-3", "plan-gtr-4-5", "plan-gtr-4-3",
             "plan-lg-1-5", "plan-lg-4-5"]
TAPE_SETS = ["tape-jc69", "tape-gtr-g4"]


@pytest.mark.parametrize("name", SAMPLER_SETS + PLAN_SETS + TAPE_SETS)
def test_the_sets_fire_at_their_start_trees(name):
    c = firing.case(name)
    firing.fires_at_start(c["data"])
    print(f"[fires] {name}: f = {c['f']:g}, (nodes, top) per locus {firing.summary(c['data'])}")
    tips = {len(s) for s in c["species"]}
    if name == "big-17":
        assert [len(s) for s in c["species"]] == [17, 17, 17, 24, 24, 24]
    elif name.startswith("plan-lg"):
        assert [len(s) for s in c["species"]] == [16] * 5 + [24]
    else:
        assert tips == {64 if name == "big-64" else 24}
    if name.startswith("plan-"):
        want = firing.P5 if name.endswith("-5") else firing.P3
        assert tuple(len(d["weights"]) for d in c["data"])[:len(want)] == want
    assert c["f"] >= 1e-6


def test_a_set_that_does_not_fire_is_refused():
    """the assertions on sequences a few percent apart (tests/shapes.py): every counter is zero, both refuse"""
    c = shapes.case("big-17-30")
    with pytest.raises(AssertionError, match="inner node"):
        firing.fires_at_start(c["data"])
    with pytest.raises(AssertionError, match="every counter is zero"):
        firing.still_fires(c["data"], c["data"])


def test_a_set_that_fires_at_its_roots_only_is_refused():
    """17 tips at 1e-6 with two or three sequences per species and without the generator's redraws: a counter at the root
    alone (no parent adds a child's count)"""
    stree = firing.scaled_species_tree(1e-6)
    rng = np.random.default_rng(3)
    found = None
    for _ in range(40):
        d = firing.firing_locus([0, 0, 0] + [k // 2 for k in range(2, 16)], stree, 30, rng=rng, nodes=0)
        (lnl, sc, root), = firing.counters([d])
        if [v for v, s in sc.items() if s.any()] == [root]:
            found = d
            break
    assert found is not None
    with pytest.raises(AssertionError, match="only the root|inner node"):
        firing.fires_at_start([found], nodes=1)
    with pytest.raises(AssertionError, match="no node other than a root"):
        firing.still_fires([found], [found])


@pytest.mark.parametrize("moves", ["uniform", "program"])
@pytest.mark.parametrize("name", SAMPLER_SETS)
def test_reference_driver_keeps_its_state_where_the_counters_fire(name, moves):
    c = firing.case(name)
    data, parent = c["data"], c["stree"][0]
    n = len(data)
    firing.fires_at_start(data)
    drv = hostdrv.reference_driver(data, seed=29, scaling=True)
    shapes.configure(drv, c, moves, host=True)
    drv.initialize()
    kw = dict(tip_species=c["species"], scaling=True)
    check_state(drv, data, parent, **kw)
    line = [firing.summary(data)]
    for it in range(1, 31):
        drv.iterate()
        if it in (3, 10, 30):
            seen = check_state(drv, data, parent, **kw)
            trees = [drv.tree(i) for i in range(n)]
            firing.still_fires(data, trees)
            line.append(firing.summary(data, trees))
            assert seen["lnl"] < 1e-12 and seen["logpr"] < 1e-11
    p, a, _ = drv.counters()
    moved(drv, c["stree"][1], c["stree"][2], p, a)
    print(f"[fires] {name} {moves}: accepted {a / p:.2f}; nodes per locus at 0 / 3 / 10 / 30: " + " / ".join(str([x[0] for x in s]) for s in line)
          + f"; largest counter {[max(x[1] for x in s) for s in line]}")
    drv.close()


@pytest.mark.parametrize("name", TAPE_SETS)
def test_the_tape_sets_still_fire_on_their_final_trees(name):
    """the proposal tape of tests/test_gpu_scaling_fires.py (3 iterations of bpp_amd.schedule on the set, its rubber-band taus
    scaled like the species tree): the counters fire on the trees it ends on, and every step of the oracle's replay — what the
    device's steps are held to — is finite"""
    c = firing.case(name)
    sch, steps = firing.tape_steps(c)
    firing.still_fires(c["data"], sch.trees)
    print(f"[fires] {name}: {len(steps)} steps; (nodes, top) per locus at the start {firing.summary(c['data'])}, on the final trees {firing.summary(c['data'], sch.trees)}")
    for li, d in enumerate(c["data"]):
        got = tape.oracle_replay(d, tape.locus_subtape(steps, li), True)
        assert len(got) > 100 and np.isfinite(got).all(), li
