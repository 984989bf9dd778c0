"""Loci of an EXACT shape (plain helper module, no fixtures): a wanted number of tips and of site patterns, for the tests
that run the device samplers at the sizes where they hand over to each other or refuse (tests/test_gpu_sampler_limits.py;
CPU twin: tests/test_host_driver_limits.py).  synth.make_dataset cannot do that: its pattern counts fall where the simulation
puts them, far inside the limits.

A locus is the dict tape.make_engine_loci, tape.ref_locus_for and the oracle take.  Its columns are pairwise distinct as
strings with weights >= 1; they are NOT a minimal compression (two columns may be relabellings of each other under JC69, or
differ only in '-' against 'N'): the locus API and the oracle take any columns with weights.
"""
import numpy as np

from bpp_amd import synth
from invariants import oracle_locus

NT = "ACGT"
AMBIGUOUS = "RYMKSWBDHVN-"                # with <= 4 tips there are too few distinct columns over ACGT alone
GTR_FREQS, GTR_EXCH = np.array([0.3, 0.2, 0.2, 0.3]), np.array([1, 2, 1, 0.5, 1.5, 1.0])      # synth.make_dataset's


def shaped_locus(tip_species, stree, npat, model="jc69", rate_cats=1, rng=None, noise=0.05, bases=4, extra=3.0):
    """One locus with exactly `npat` columns on len(tip_species) tips.

    tip_species: the species of every tip; stree: (parent, tau, theta) of the species tree.  The start tree comes from
    synth.msc_start_tree, so it is MSC-valid.  Columns: `bases` base columns give every SPECIES a letter that follows the
    species tree (a child population keeps its parent's letter two times in three), a site is a base column with every tip's
    letter replaced with probability `noise` (as invariants.several_sequences_data) — sites are drawn until `npat` distinct
    columns exist, then `extra` x as many more that only add weight to the columns already there, so the likelihood has
    signal.  Where the draws stop giving new columns (few tips, many patterns) the noise grows."""
    rng = np.random.default_rng(1) if rng is None else rng
    parent, tau, theta = stree
    tips, npop = len(tip_species), len(parent)
    left, right, times, root = synth.msc_start_tree(list(tip_species), parent, tau, theta, rng)
    alphabet = list(NT + AMBIGUOUS) if tips <= 4 else list(NT)
    base_cols = []
    for _ in range(bases):
        letter = [None] * npop
        for p in range(npop - 1, -1, -1):                 # parents come after their children: root first
            up = None if parent[p] < 0 else letter[parent[p]]
            letter[p] = up if up is not None and rng.random() < 2 / 3 else str(rng.choice(list(NT)))
        base_cols.append(np.array([letter[s] for s in tip_species]))
    weight, stale, level = {}, 0, noise

    def site():
        col = base_cols[rng.integers(bases)]
        return "".join(np.where(rng.random(tips) > level, col, rng.choice(alphabet, tips)))

    while len(weight) < npat:
        c = site()
        if c in weight:
            stale += 1
            if stale % 40 == 0:
                level = min(1.0, level * 1.5)
        weight[c] = weight.get(c, 0) + 1
    level = noise
    for _ in range(int(extra * npat)):
        c = site()
        if c in weight:
            weight[c] += 1
    cols = list(weight)
    d = dict(seqs=["".join(c[k] for c in cols) for k in range(tips)], weights=np.array([weight[c] for c in cols], dtype=np.uint32),
             left=left, right=right, times=times, root=root, states=4, rate_cats=rate_cats, model=model,
             rates=synth._discrete_gamma(0.5, rate_cats))
    if model != "jc69":
        d["freqs"], d["exch"] = GTR_FREQS.copy(), GTR_EXCH.copy()
    assert len(cols) == npat == len(set(cols)) == len(d["seqs"][0]) and d["weights"].min() >= 1, (npat, len(cols))
    lnl = oracle_locus(d, None, None, False, None).full_lnl(list(left), list(right), list(times), root)
    assert np.isfinite(lnl), (tips, npat, lnl)
    return d


def shaped_set(tip_species, stree, counts, seed, **kw):
    """one locus per entry of `counts`, in that order, all on the same tips"""
    rng = np.random.default_rng(seed)
    return [shaped_locus(tip_species, stree, n, rng=rng, **kw) for n in counts]


def waves(counts, lpw):
    """what the persistent kernel's packing does to a list of pattern counts (csrc/sampler.hpp: sampler_upload_v2 closes a
    wave with `cnt == LPW || used + np > 64`; lpw = 8 in the 4-tip form, 4 in the 8-tip form) -> the waves' count lists"""
    out, cur = [], []
    for n in counts:
        if len(cur) == lpw or sum(cur) + n > 64:
            out.append(cur); cur = []
        cur.append(n)
    out.append(cur)
    return out


def blocks(counts, bs=64, tpb=16):
    """the same for the one-launch-per-step path (csrc/sampler.hpp: sampler_upload, `used + np > BS || ntask == TPB`)"""
    out, cur = [], []
    for n in counts:
        if sum(cur) + n > bs or len(cur) == tpb:
            out.append(cur); cur = []
        cur.append(n)
    out.append(cur)
    return out


# ---------------------------------------------------------------- the shaped sets of the limit tests, built once per process
# pattern counts per locus, in sampler order.  4-tip form of the persistent kernel (8 loci per wave):
COUNTS4 = (1, 8, 9, 15, 16, 17, 25, 33, 63, 64, 64, 1, 1, 1, 1, 1, 1, 1, 1, 57, 7, 8, 8, 8, 8, 8, 8, 8, 8, 40, 24, 25, 9, 9, 9, 9, 9, 9, 9, 2)
# 8-tip form (4 loci per wave); the six counts after the 5 were added to the issue's list: without them no wave of this form
# reaches exactly 64 patterns with exactly 4 loci
COUNTS8 = (1, 16, 17, 32, 33, 48, 49, 63, 64, 64, 1, 1, 1, 1, 30, 34, 5) + (59, 16, 16, 16, 16, 3)
TWO_SPECIES = ([2, 2, -1], [0.0, 0.0, 0.003], [0.002, 0.003, 0.004])          # invariants.several_sequences_data's species tree
LAYOUTS = ((1, 1), (2, 1), (2, 2), (3, 2), (4, 3), (4, 4))                    # sequences per species: 2, 3, 4, 5, 7, 8 tips

def packing(counts, lpw):
    """what the list does to the packing, worked out on the host -> the waves; asserts the shapes the list is there for"""
    w = waves(counts, lpw)
    G = 64 // lpw
    assert sum(map(len, w)) == len(counts) and all(1 <= len(x) <= lpw and sum(x) <= 64 for x in w)
    assert any(len(x) < lpw and sum(x) + w[k + 1][0] > 64 for k, x in enumerate(w[:-1])), "no wave closes on patterns with idle lane groups"
    assert any(len(x) == lpw and sum(x) == 64 for x in w), "no full wave of exactly 64 patterns"
    assert any(x == [64] and w[k + 1][0] == 1 for k, x in enumerate(w[:-1])), "no one-locus 64-pattern wave followed by one-pattern loci"
    assert any(sum(x[:j]) > 0 and x[j] > G for x in w for j in range(len(x))), "no locus of several passes behind a non-zero first slot"
    assert len(w) > 4, "the waves fit one workgroup (4 waves with loci at the most): no sum crosses workgroups"
    return w


def check_lists():
    """COUNTS4 and COUNTS8 against both packings, on the host"""
    w4, w8 = packing(COUNTS4, 8), packing(COUNTS8, 4)
    assert w4[0] == [1, 8, 9, 15, 16] and [64] in w4 and [1] * 8 in w4 and [8] * 8 in w4 and len(w4) == 12
    assert w8[0] == [1, 16, 17] and [1, 1, 1, 1] in w8 and [16] * 4 in w8
    assert max(COUNTS4) == max(COUNTS8) == 64 and min(COUNTS4) == min(COUNTS8) == 1
    # passes of the pattern loop (G lanes a pass): one, two, three and the last (8 in the 4-tip form, 4 in the 8-tip form)
    assert {-(-n // 8) for n in COUNTS4} >= {1, 2, 3, 4, 5, 8} and {-(-n // 16) for n in COUNTS8} == {1, 2, 3, 4}
    for counts in (COUNTS4, COUNTS8):
        b = blocks(counts)
        assert any(len(x) < 16 and sum(x) + b[k + 1][0] > 64 for k, x in enumerate(b[:-1])) and [64] in b


_SETS = {}


def _case(name, data, species, stree, kind, **kw):
    parent, tau0, thetas = stree
    c = dict(name=name, data=data, species=species, stree=stree, kind=kind, scaling=False, subst=False, slide=0.3,
             tau_prior=(3.0, 3.0 / tau0[-1]), theta_prior=(2.0, 1000.0, 0.0004), finetune=(0.003, 0.004, 0.0004, 0.1))
    c.update(kw)
    return c


def _build(name):
    st4, st8 = synth.species_tree_arrays(4), synth.species_tree_arrays(8)
    one4, one8 = list(range(4)), list(range(8))
    two16 = [k // 2 for k in range(16)]
    several = dict(tau_prior=(3.0, 1000.0), theta_prior=(2.0, 700.0, 0.002), finetune=(0.003, 0.004, 0.0008, 0.2), slide=0.5)
    if name == "persistent-4":
        d = shaped_set(one4, st4, COUNTS4, 11)
        return _case(name, d, [one4] * len(d), st4, "persistent")
    if name == "persistent-8":
        d = shaped_set(one8, st8, COUNTS8, 12)
        return _case(name, d, [one8] * len(d), st8, "persistent")
    if name == "persistent-mixed-tips":
        # 2, 3, 4, 5, 7 and 8 tips in ONE sampler, at 20 and at 40 patterns, two loci of each; the tip populations hold coalescences
        rng = np.random.default_rng(13)
        d, sp = [], []
        for rep in range(2):
            for npat in (20, 40):
                for a, b in LAYOUTS:
                    sp.append([0] * a + [1] * b)
                    d.append(shaped_locus(sp[-1], TWO_SPECIES, npat, rng=rng))
        return _case(name, d, sp, TWO_SPECIES, "persistent", **several)
    if name == "handover-65":
        # COUNTS4 with its first 64-pattern locus at 65: one locus beyond the LDS kernels makes the whole set the generic sampler's
        counts = list(COUNTS4)
        counts[counts.index(64)] = 65
        d = shaped_set(one4, st4, counts, 11)
        return _case(name, d, [one4] * len(d), st4, "generic")
    if name == "composite-64-65":
        # 64- and 65-pattern 8-tip JC69 loci in turns (64 of each: a part of the LDS kernels' needs 64 loci, csrc/composite.hpp) and
        # six GTR+Gamma4 loci in between
        rng = np.random.default_rng(14)
        d = []
        for i in range(64):
            d.append(shaped_locus(one8, st8, 64, rng=rng))
            d.append(shaped_locus(one8, st8, 65, rng=rng))
            if i % 11 == 0:
                d.append(shaped_locus(one8, st8, 40, "gtr", 4, rng=rng))
        return _case(name, d, [one8] * len(d), st8, "composite", theta_prior=(2.0, 1000.0, 0.001), finetune=(0.003, 0.005, 0.0008, 0.2))
    if name == "generic-16-jc":
        d = shaped_set(two16, st8, (1, 64, 200, 255), 15)
        return _case(name, d, [two16] * len(d), st8, "generic")
    if name == "generic-16-gtr-g4":
        d = shaped_set(two16, st8, (63,) * 5, 16, model="gtr", rate_cats=4)                  # 252 lanes
        return _case(name, d, [two16] * len(d), st8, "generic", subst=True)
    if name == "generic-16-gtr-g3":
        d = shaped_set(two16, st8, (85,) * 5, 17, model="gtr", rate_cats=3)                  # 255 lanes
        return _case(name, d, [two16] * len(d), st8, "generic")
    if name == "generic-16-gtr-g8":
        d = shaped_set(two16, st8, (31,) * 5, 18, model="gtr", rate_cats=8)                  # 248 lanes
        return _case(name, d, [two16] * len(d), st8, "generic")
    if name == "generic-12-and-16":
        rng = np.random.default_rng(19)
        two12 = [k // 2 for k in range(12)]
        d, sp = [], []
        for npat in (30, 100, 60):
            for s in (two12, two16):
                sp.append(s)
                d.append(shaped_locus(s, st8, npat, rng=rng))
        return _case(name, d, sp, st8, "generic")
    if name.startswith("big-"):
        # big-<tips>-<patterns>: 8 species; 17 tips = three sequences of species 0 and two of the others, 64 = eight of each
        _, tips, npat = name.split("-")
        s = [0, 0, 0] + [k // 2 for k in range(2, 16)] if tips == "17" else [k // 8 for k in range(64)]
        assert len(s) == int(tips)
        d = shaped_set(s, st8, (int(npat),) * 3, 20 + int(tips) + int(npat))
        return _case(name, d, [s] * 3, st8, "big", theta_prior=(2.0, 500.0, 0.001), finetune=(0.002, 0.003, 0.0004, 0.1))
    raise KeyError(name)


SMALL = ("persistent-4", "persistent-8", "persistent-mixed-tips", "handover-65", "composite-64-65", "generic-16-jc",
         "generic-16-gtr-g4", "generic-16-gtr-g3", "generic-16-gtr-g8", "generic-12-and-16")           # <= 16 tips
BIG = tuple(f"big-{t}-{n}" for t in (17, 64) for n in (30, 300))


def case(name):
    """the named set (a dict: data, species per locus, stree, kind, priors, step lengths); built once, never changed"""
    if name not in _SETS:
        _SETS[name] = _build(name)
    return _SETS[name]


OPTION_IDS = {"one_call": "ONE_CALL", "chain": "BPA_GS_CHAIN", "host_decisions": "BPA_GS_HOSTDEC"}


def option_id(v):
    """ids= of a parametrisation whose cases carry bpp_amd.Sampler options as a dict (next to test-side switches such as
    one_call): the name the case has always had, that of the variable the option's default is read from"""
    if not isinstance(v, dict):
        return None
    return "+".join(OPTION_IDS[k] if k == "one_call" else f"{OPTION_IDS[k]}={int(x)}" for k, x in v.items())


def configure(drv, c, moves, host=False):
    """species tree, tips' species, priors, step lengths and the moves ('uniform', 'bpp', 'program') of case c on a
    hostdrv.Driver (host=True) or a bpp_amd.Sampler — the same calls on both, so that they walk the same chain"""
    parent, tau0, thetas = c["stree"]
    if moves != "uniform":
        drv.set_proposal_kernel(1)
    if moves == "program":
        drv.set_program_moves(True, c["slide"])
    drv.set_species_tree(parent, tau0, thetas)
    for i, s in enumerate(c["species"]):
        drv.set_tip_species(i, s)
    drv.set_tau_prior(*c["tau_prior"])
    drv.set_theta_prior(*c["theta_prior"])
    drv.set_finetune(*c["finetune"])
    if c["subst"]:
        drv.set_subst_moves(0.3, 0.4, 0.8, 1.0, 1.0)
        for i, d in enumerate(c["data"]):
            if host:
                drv.set_subst_model(i, list(d["freqs"]), list(d["exch"]), 0.5, d["rate_cats"])
            else:
                drv.set_subst_model(i, d["freqs"], d["exch"], 0.5)
