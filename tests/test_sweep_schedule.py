"""The persistent kernel's sweep schedule (bpa_sweep_schedule, csrc/sampler.hpp; what it means: csrc/sweep2.hpp, Sched): which
wave of a workgroup runs which steps of which set of loci.  Host code, no GPU: for 4 .. 8 waves of loci and 1 .. 9 steps a sweep

 * every set's steps are run exactly once and in order, by one wave at a time;
 * no wave is asked to hold two sets, no set is taken by two waves;
 * the waits (a wave takes a set only after its previous holder parked it) form no cycle;
 * an event simulation with the two measured step costs — 20.8 k cycles for a wave that has its SIMD's issue slots, 33 k for the
   younger wave of a pair while the older one runs — ends, and not later than the identity schedule's.
"""
import ctypes

import pytest

import bpp_amd

FAST, SLOW = 20.8, 33.0
SEGS = 4


def schedule(lwaves, steps, hand_overs, fast=FAST, slow=SLOW):
    buf = ctypes.create_string_buffer(68)
    nseg = bpp_amd.lib().bpa_sweep_schedule(lwaves, steps, fast, slow, hand_overs, buf)
    raw = buf.raw
    src = [[raw[4 + r * SEGS + k] for k in range(SEGS)] for r in range(8)]
    n = [[raw[36 + r * SEGS + k] for k in range(SEGS)] for r in range(8)]
    return dict(ret=nseg, nseg=raw[0], nroles=raw[1], npairs=raw[2], src=src, n=n)


def seg_steps(sc, steps, r, k, done):
    """steps role r runs in segment k on a set that has `done` behind it: the table's count, the last segment all that are left"""
    if k + 1 < sc["nseg"] and done + sc["n"][r][k] < steps:
        return sc["n"][r][k]
    return steps - done


def walk(sc, steps):
    """the sets through the segments; returns per set the list of (role, first step, steps run)"""
    R = sc["nroles"]
    holds = list(range(R))                       # holds[r] = the set role r holds
    done = [0] * R
    runs = [[] for _ in range(R)]
    for k in range(sc["nseg"]):
        if k:
            takers = [r for r in range(R) if sc["src"][r][k] != r]
            givers = sorted(sc["src"][r][k] for r in takers)
            assert givers == sorted(takers), (k, takers, givers)        # whoever takes a set gives its own; nobody gives twice
            assert all(g < R for g in givers)
            holds = [holds[sc["src"][r][k]] for r in range(R)]
        assert sorted(holds) == list(range(R)), (k, holds)              # a wave holds one set, a set has one holder
        for r in range(R):
            s = holds[r]
            m = seg_steps(sc, steps, r, k, done[s])
            assert m >= 0
            if m:
                runs[s].append((r, done[s], m))
            done[s] += m
    assert done == [steps] * R
    return runs


def simulate(sc, steps, fast=FAST, slow=SLOW):
    """events: a lane runs its segment's steps one after the other; at a segment's end it parks its set and waits until the
    set it takes has been parked.  The younger lane of a pair (odd places behind the alone lanes) pays `slow` a step while
    its older partner runs a step, `fast` otherwise.  Returns the time the last lane finishes."""
    R, nalone = sc["nroles"], sc["nroles"] - 2 * sc["npairs"]
    seg = [0] * R; holds = list(range(R)); done = [0] * R
    left = [seg_steps(sc, steps, r, 0, 0) for r in range(R)]
    frac = [0.0] * R; waiting = [False] * R; fin = [False] * R
    parked = {}
    t = 0.0
    for _ in range(10000):
        moved = True
        while moved:
            moved = False
            for r in range(R):
                if fin[r]:
                    continue
                if not waiting[r] and left[r] == 0:
                    if seg[r] + 1 >= sc["nseg"]:
                        fin[r] = True; moved = True
                        continue
                    seg[r] += 1
                    if sc["src"][r][seg[r]] != r:
                        parked[(r, seg[r])] = holds[r]; holds[r] = None; waiting[r] = True
                    else:
                        left[r] = seg_steps(sc, steps, r, seg[r], done[holds[r]])
                    moved = True
                if waiting[r] and (sc["src"][r][seg[r]], seg[r]) in parked:
                    holds[r] = parked.pop((sc["src"][r][seg[r]], seg[r])); waiting[r] = False
                    left[r] = seg_steps(sc, steps, r, seg[r], done[holds[r]])
                    moved = True
        running = [r for r in range(R) if not fin[r] and not waiting[r] and left[r] > 0]
        if not running:
            assert all(fin), "a wave waits for a set that nobody parks"
            assert done == [steps] * R
            return t
        cost = {}
        for r in running:
            young = r >= nalone and (r - nalone) % 2 == 1
            cost[r] = slow if young and (r - 1) in running else fast
        dt = min((1.0 - frac[r]) * cost[r] for r in running)
        t += dt
        for r in running:
            frac[r] += dt / cost[r]
            if frac[r] >= 1.0 - 1e-12:
                frac[r] = 0.0; left[r] -= 1; done[holds[r]] += 1
    raise AssertionError("the simulation does not end")


@pytest.mark.parametrize("hand_overs", [0, 1, 2, 3])
@pytest.mark.parametrize("steps", range(1, 10))
@pytest.mark.parametrize("lwaves", range(4, 9))
def test_schedule(lwaves, steps, hand_overs):
    sc = schedule(lwaves, steps, hand_overs)
    assert sc["ret"] == sc["nseg"] and 1 <= sc["nseg"] <= SEGS
    assert sc["nroles"] == lwaves and sc["npairs"] == max(lwaves - 4, 0)
    runs = walk(sc, steps)
    for s, rr in enumerate(runs):
        at = 0
        for (_role, first, m) in rr:                 # in order, nothing twice, nothing left out
            assert first == at
            at += m
        assert at == steps, (s, rr)
    # the wait graph: (r, k) = "role r begins segment k" needs r's and its giver's segment k - 1 — no cycle
    need = {(r, k): ({(r, k - 1), (sc["src"][r][k], k - 1)} if k else set()) for r in range(lwaves) for k in range(sc["nseg"])}
    order = []
    while need:
        free = [v for v, d in need.items() if not d]
        assert free, "the waits form a cycle"
        for v in free:
            del need[v]
        for d in need.values():
            d.difference_update(free)
        order += free
    ident = schedule(lwaves, steps, 0)
    assert ident["nseg"] == 1 and all(ident["src"][r][0] == r and ident["n"][r][0] == steps for r in range(lwaves))
    t, t_id = simulate(sc, steps), simulate(ident, steps)
    assert t <= t_id + 1e-9, (t, t_id)
    if lwaves <= 4:
        assert abs(t_id - steps * FAST) < 1e-9
    if hand_overs == 0:
        assert sc["nseg"] == 1


def test_the_headline_case_hands_over_and_gains():
    """5 waves of loci, 9 steps a sweep (four tips: 3 age moves + 6 prune-and-regraft moves).  Identity: the older wave is done
    after 9 x 20.8 = 187 k, the younger has 5.7 steps behind it by then and runs the other 3.3 fast: 256 k.  A chain of three
    swaps: the younger wave runs one step each of its own and the three alone waves' sets and finishes the last; every
    alone wave runs a step more than a sweep's: ~ 10 x 20.8 = 208 k + what the waits cost"""
    t0 = simulate(schedule(5, 9, 0), 9)
    assert abs(t0 - (9 * FAST + (9 - 9 * FAST / SLOW) * FAST)) < 1e-6
    three = schedule(5, 9, 3)
    assert three["nseg"] == 4
    assert [three["src"][4][k] for k in (1, 2, 3)] == [0, 1, 2] and [three["src"][a][a + 1] for a in (0, 1, 2)] == [4, 4, 4]
    assert [three["n"][4][k] for k in (0, 1, 2)] == [1, 1, 1]
    assert three["src"][3] == [3, 3, 3, 3] and three["n"][3][0] == 9            # the older wave of the pair keeps its set
    t3 = simulate(three, 9)
    assert t3 < 0.86 * t0 and t3 >= 45 / (4 / FAST + 1 / SLOW), (t3, t0)      # (45 steps on four fast lanes and a slow one at best)
    t1, t2 = simulate(schedule(5, 9, 1), 9), simulate(schedule(5, 9, 2), 9)
    assert t3 < t2 < t1 < t0, (t3, t2, t1, t0)


def test_arguments_out_of_range():
    buf = ctypes.create_string_buffer(68)
    L = bpp_amd.lib()
    assert L.bpa_sweep_schedule(0, 5, FAST, SLOW, 1, buf) == 0
    assert L.bpa_sweep_schedule(9, 5, FAST, SLOW, 1, buf) == 0
    assert L.bpa_sweep_schedule(5, 0, FAST, SLOW, 1, buf) == 0
    assert L.bpa_sweep_schedule(5, 5, SLOW, FAST, 1, buf) == 0      # the younger wave is never the faster
    assert L.bpa_sweep_schedule(5, 5, FAST, SLOW, 4, buf) == 0
