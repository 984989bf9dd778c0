"""Loci whose per-pattern scale counters are NOT zero (plain helper module, no fixtures), for the tests of every code path that
takes `scaling=True`: batched plans, tapes, the C host driver and the big-tree sampler (tests/test_gpu_scaling_fires.py; CPU twin:
tests/test_scaling_fires.py).  shapes.shaped_locus and synth.make_dataset give sequences a few percent apart on trees of normal
depth: every counter of theirs stays 0 and `0 == 0` is what a scaling test then compares.

Recipe: columns in which every tip's letter is drawn independently (a mismatch at every coalescence), on a start tree from
synth.msc_start_tree under synth.species_tree_arrays(8) with every tau and theta multiplied by a factor f << 1 (every mismatch
then costs a factor of about the branch length, and 2^-256 is reached within a few nodes).  The priors and step lengths of a
case are scaled by f as well, so that a chain stays where the counters fire.

A case proves what it needs about its own input with the assertions below — from the ORACLE's recompute alone, never from a
device buffer:
  fires_at_start   every locus: finite lnL with scale buffers; >= `nodes` inner nodes with a non-zero counter, one of them not the
                   root (else no parent ever adds a child's count).  Over the set: some node with both zero and non-zero counters
                   among its patterns (else per-pattern indexing is never exercised), and some counter >= 2.
  still_fires      every locus: finite lnL, a non-zero counter at some inner node.  Over the set: one at a node that is no root.
"""
import numpy as np

from bpp_amd import synth
import shapes
from invariants import oracle_locus

NT, AA = "ACGT", "ARNDCQEGHILKMFPSTWYV"
# The tips' species.  A node below the root fires where ten or so tips meet within a few 1e-9: with two or three sequences per
# species that depends on the shape a tree happens to have, and a chain loses it at every other checkpoint (measured with the
# reference-API driver: of six 24-tip loci with three sequences per species, none had a firing node below the root at 3 of 48
# checkpoints under JC69 and at 2 of 48 under GTR+Gamma4).  Ten sequences of one species coalesce inside its population and fire
# there in nearly every tree.
S17 = [0] * 10 + list(range(1, 8))
S24 = [0] * 10 + [1] * 8 + list(range(2, 8))
S16 = [k // 2 for k in range(16)]
S64 = [k // 8 for k in range(64)]


def scaled_species_tree(f, taxa=8):
    """synth.species_tree_arrays(taxa) with every tau and theta multiplied by f"""
    parent, tau, theta = synth.species_tree_arrays(taxa)
    return parent, [t * f for t in tau], [t * f for t in theta]


def firing_locus(tip_species, stree, npat, states=4, model="jc69", rate_cats=1, rng=None, nodes=2, draws=400):
    """one locus of exactly `npat` pairwise distinct columns, every tip's letter drawn independently, weights 1..8; the start tree
    from synth.msc_start_tree on `stree`.  The dict tape.make_engine_loci, tape.ref_locus_for and the oracle take.

    A one-pattern locus has two nodes with a counter only where its one column underflows below the root, which few draws
    give: tree and columns are drawn again (from the same generator, so a seed still fixes the locus) until the oracle finds
    a finite lnL and a non-zero counter at `nodes` inner nodes or more, one of them not the root — the locus's own part of
    fires_at_start, which the tests assert again on what comes out; `draws` draws without one is an error."""
    rng = np.random.default_rng(1) if rng is None else rng
    parent, tau, theta = stree
    tips = len(tip_species)
    alphabet = list(NT if states == 4 else AA)
    for _ in range(draws):
        left, right, times, root = synth.msc_start_tree(list(tip_species), parent, tau, theta, rng)
        cols = set()
        while len(cols) < npat:
            cols.add("".join(rng.choice(alphabet, tips)))
        cols = sorted(cols)
        d = dict(seqs=["".join(c[k] for c in cols) for k in range(tips)], weights=rng.integers(1, 9, npat).astype(np.uint32),
                 left=left, right=right, times=times, root=root, states=states, rate_cats=rate_cats, model=model,
                 rates=synth._discrete_gamma(0.5, rate_cats))
        if model == "gtr":
            d["freqs"], d["exch"] = shapes.GTR_FREQS.copy(), shapes.GTR_EXCH.copy()
        elif model == "lg":
            d["exch"], d["freqs"] = synth.lg_model()
        lnl, sc = fires(oracle_locus(d, None, None, True, None), _tree(None, d))
        hot = [v for v, s in sc.items() if s.any()]
        if np.isfinite(lnl) and (nodes == 0 or (len(hot) >= nodes and any(v != root for v in hot))):      # (0: the first draw)
            return d
    raise AssertionError(f"{tips} tips, {npat} patterns, {model}: no locus with {nodes} firing nodes in {draws} draws")


def firing_case(name, tip_species, f, counts, seed, states=4, model="jc69", rate_cats=1, kind="big", nodes=2):
    """a set of len(counts) loci -> the dict of shapes.case (data, species, stree, priors, step lengths; shapes.configure sets a
    driver or a sampler up from it), with scaling=True and the factor under 'f'.  tip_species: the tips' species, the same for
    every locus, or a list of them, one per locus; nodes: firing_locus's, likewise.

    Priors and step lengths follow the species tree, all x f.  Random columns pull every age up (each mismatch wants a longer
    branch), and a chain that follows them leaves the region where the counters fire within some tens of iterations: the priors
    are therefore narrow (tau: gamma(300) with the start tree's root tau as its mean; theta: gamma(200) with the start tree's
    theta as its mean) and the steps a tenth of tests/shapes.py's for the big-tree sampler, the MIX move's included."""
    stree = scaled_species_tree(f)
    rng = np.random.default_rng(seed)
    sp = [list(tip_species)] * len(counts) if isinstance(tip_species[0], int) else [list(s) for s in tip_species]
    nd = [nodes] * len(counts) if isinstance(nodes, int) else list(nodes)
    data = [firing_locus(sp[k], stree, n, states, model, rate_cats, rng, nd[k]) for k, n in enumerate(counts)]
    # a counter of 2 takes two underflows on one path: where the set has none, its last locus is drawn again (fires_at_start's
    # condition over the set, asserted again by the tests)
    top = max(hi for _, hi in summary(data[:-1])) if len(data) > 1 else 0
    for _ in range(300):
        if max(top, summary(data[-1:])[0][1]) >= 2:
            break
        data[-1] = firing_locus(sp[-1], stree, counts[-1], states, model, rate_cats, rng, nd[-1])
    else:
        raise AssertionError(f"{name}: no counter >= 2 in 300 draws of the last locus")
    g = 0.1 * f
    return dict(name=name, data=data, species=sp, stree=stree, kind=kind, scaling=True, subst=False, slide=0.3, f=f,
                tau_prior=(300.0, 300.0 / stree[1][-1]), theta_prior=(200.0, 200.0 / stree[2][-1], 0.001 * g),
                finetune=(0.002 * g, 0.003 * g, 0.0004 * g, 0.01))


def _tree(t, d):
    """(left, right, times, root) of a driver's / sampler's tree dict, a schedule's TreeState, or None: the locus's start tree"""
    if t is None:
        t = d
    get = t.get if isinstance(t, dict) else lambda k, default=None: getattr(t, k, default)
    nn = 2 * len(d["seqs"]) - 1
    times = get("time") if get("time") is not None else get("times")
    return ([int(x) for x in get("left")][:nn], [int(x) for x in get("right")][:nn], [float(x) for x in times][:nn], int(get("root")))


def fires(ol, tree):
    """the oracle's recompute of `tree` = (left, right, times, root) on locus `ol` (an OracleLocus with scaling=True) ->
    (lnL, {inner node: its counters per pattern})"""
    left, right, times, root = tree
    lnl = ol.full_lnl(left, right, times, root)
    return lnl, {v: ol.scaler[v] for v in range(len(left)) if left[v] >= 0}


def counters(data, trees=None):
    """per locus (lnL, {inner node: counters}, root) from the oracle on trees[i] (None: the start trees)"""
    out = []
    for i, d in enumerate(data):
        tr = _tree(None if trees is None else trees[i], d)
        lnl, sc = fires(oracle_locus(d, None, None, True, None), tr)
        out.append((lnl, sc, tr[3]))
    return out


def summary(data, trees=None):
    """per locus (nodes with a non-zero counter, largest counter): what the tables of the tests' headers quote"""
    return [(sum(bool(s.any()) for s in sc.values()), max(int(s.max()) for s in sc.values())) for _, sc, _ in counters(data, trees)]


def fires_at_start(data, trees=None, nodes=2):
    """conditions 1 and 2 of the module header"""
    mixed, top = False, 0
    for i, (lnl, sc, root) in enumerate(counters(data, trees)):
        assert np.isfinite(lnl), f"locus {i}: lnL {lnl} with scale buffers"
        hot = [v for v, s in sc.items() if s.any()]
        assert len(hot) >= nodes, f"locus {i}: {len(hot)} inner node(s) with a non-zero counter, {nodes} wanted"
        assert any(v != root for v in hot), f"locus {i}: only the root has a non-zero counter"
        mixed = mixed or any(s.any() and not s.all() for s in sc.values())
        top = max(top, max(int(s.max()) for s in sc.values()))
    assert mixed, "no node has both zero and non-zero counters among its patterns"
    assert top >= 2, f"the largest counter of the set is {top}"


def still_fires(data, trees):
    """conditions 1 and 3 of the module header"""
    below = False
    for i, (lnl, sc, root) in enumerate(counters(data, trees)):
        assert np.isfinite(lnl), f"locus {i}: lnL {lnl} with scale buffers"
        hot = [v for v, s in sc.items() if s.any()]
        assert hot, f"locus {i}: every counter is zero"
        below = below or any(v != root for v in hot)
    assert below, "no node other than a root has a non-zero counter"


# ---------------------------------------------------------------- the named sets, built once per process and never changed
_SETS = {}
P5 = (1, 63, 64, 65, 193)                  # pattern counts of a batch: one lane, around a wave, beyond 64 and 128
P3 = (1, 63, 64)                           # ... with none beyond 64: the batch's workgroup size is then 64 (engine.hip: plan_build)


def _build(name):
    if name == "big-17":
        # 17 tips fire once on any path at f = 1e-6 (sixteen mismatches of 1e-10 ... 1e-9 each do not reach 2^-512): no draw of
        # 300 gave a counter of 2, with any of the three layouts of the species tried (3 + 7 x 2, 11 + 6 x 1, 10 + 7 x 1).  That condition over the set is met by the three 24-tip loci
        # that run in the same sampler; every 17-tip locus itself starts with two firing nodes or more, as the others do
        return firing_case(name, [S17] * 3 + [S24] * 3, 1e-6, (30, 65, 30, 65, 30, 65), 117)
    if name == "big-24":
        return firing_case(name, S24, 1e-6, (30, 65, 30, 65, 30, 65), 124)
    if name == "big-24-gtr-g4":
        return firing_case(name, S24, 1e-6, (30, 65, 30, 65, 30, 65), 125, model="gtr", rate_cats=4)
    if name == "big-64":
        return firing_case(name, S64, 1e-3, (30, 30, 30), 164)
    if name.startswith("plan-"):
        # plan-<model>-<categories>-<5|3>: 24 tips at f = 1e-6 (20 states: 16 tips), pattern counts P5 or P3
        _, model, R, which = name.split("-")
        counts = P5 if which == "5" else P3
        if model == "lg":
            # 16 tips: at f = 1e-2 no draw of 400 gave a one-pattern locus with a firing node below the root, at 1e-4 every
            # draw of 20 patterns has one: 1e-4 is the mildest factor of 1e-2, 1e-4, 1e-6 that meets the conditions.  No 16-tip
            # draw at any of them reached a counter of 2 (as at 17 tips under JC69): a 24-tip locus in the same batch does
            return firing_case(name, [S16] * len(counts) + [S24], 1e-4, counts + (65,), 200 + int(R), states=20, model="lg",
                               rate_cats=int(R), kind="plan")
        return firing_case(name, S24, 1e-6, counts, 210 + 10 * int(R) + len(counts) + len(model), model=model, rate_cats=int(R), kind="plan")
    if name in ("tape-jc69", "tape-gtr-g4"):
        kw = {} if name == "tape-jc69" else dict(model="gtr", rate_cats=4)
        return firing_case(name, S24, 1e-6, (30, 65, 1, 64), 300 + len(name), kind="tape", **kw)
    raise KeyError(name)


def tape_steps(c, seed=4, iterations=3):
    """the proposal tape of tests/test_gpu_tape.py on a firing set -> (schedule, steps): the start-up step and `iterations` A00
    iterations with scale buffers; the schedule's rubber-band taus are that test's for 8 species, x f"""
    import tape
    sch = tape.make_schedule(c["data"], seed=seed, scaling=True, taus=tuple(t * c["f"] for t in (0.0011, 0.0025, 0.005)))
    steps = [sch.initial_step()]
    for _ in range(iterations):
        steps += sch.iteration()
    return sch, steps


def case(name):
    """the named set (the dict of firing_case); built once, never changed"""
    if name not in _SETS:
        _SETS[name] = _build(name)
    return _SETS[name]
