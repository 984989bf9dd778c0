"""SURVEY.md section 8(e) for the device-resident sampler: loci sharded over ranks, ONE all-reduced double per
all-loci step (THETA, TAU, MIX), nothing else exchanged; same seed on every rank.  Two ranks (sharing the test
box's single GPU, gloo) must walk the single-rank trajectory: same taus, thetas, gene trees."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(world, out, port, **extra):
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_sampler_worker.py"), out], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [json.load(open(f"{out}.{r}.json")) for r in range(world)]


def test_two_ranks_walk_the_single_rank_trajectory(tmp_path):
    one = run(1, str(tmp_path / "one"), 29611)[0]
    two = run(2, str(tmp_path / "two"), 29612 + os.getpid() % 500)
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-10, atol=0) and r["taus"] != [0, 0, 0, 0, 0.001, 0.002, 0.003]
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-10, atol=0)
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]      # replicated decisions
    times = two[0]["times"] + two[1]["times"]
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert len(times) == len(one["times"])
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=1e-10, atol=0)
    assert np.allclose(lnl, one["lnl"], rtol=1e-10, atol=0)
    tot = sum(r["summary"]["total_lnl"] for r in two)
    assert abs(tot - one["summary"]["total_lnl"]) < 1e-9 * abs(tot)


def test_ranks_with_different_sampling_configurations(tmp_path):
    """which populations can hold a coalescence (and so get a THETA step, two draws of the shared global stream each) is
    a property of ALL loci: here species 0 has two sequences only in rank 0's loci and species 1 only in rank 1's —
    the mask is OR-ed over the ranks at upload, so both ranks keep drawing the same numbers and walk the single-rank
    trajectory"""
    one = run(1, str(tmp_path / "one"), 29711, DIST_MIXED="1")[0]
    two = run(2, str(tmp_path / "two"), 29712 + os.getpid() % 500, DIST_MIXED="1")
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-10, atol=0)
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-10, atol=0)
    # both tip species' thetas moved (a rank without such loci still takes part in their steps)
    assert one["thetas"][0] != 0.002 and one["thetas"][1] != 0.002 and one["thetas"][2] == 0.002
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert np.allclose(lnl, one["lnl"], rtol=1e-10, atol=0)


def test_two_ranks_generic_sampler_with_parameter_moves(tmp_path):
    """the generic sampler (8 taxa, GTR + Gamma4, frequency / exchangeability / alpha moves: csrc/gsampler.hpp) sharded over
    two ranks walks the single-rank trajectory: the per-locus moves need no exchange, the all-loci steps one sum each"""
    one = run(1, str(tmp_path / "one"), 29811, DIST_GTR="1")[0]
    two = run(2, str(tmp_path / "two"), 29812 + os.getpid() % 500, DIST_GTR="1")
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-10, atol=0) and r["taus"][8:] != [0.001, 0.0012, 0.0025, 0.0011, 0.0013, 0.003, 0.005]
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-10, atol=0)
    times = two[0]["times"] + two[1]["times"]
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert len(times) == len(one["times"])
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=1e-10, atol=0)
    assert np.allclose(lnl, one["lnl"], rtol=1e-10, atol=0)


def test_two_ranks_generic_sampler_with_the_program_s_moves(tmp_path):
    """BPP's own iteration on the generic sampler over two ranks: the per-locus kernels draw BPP's windows, the host of EVERY rank
    takes the THETA / TAU / MIX decisions from the sums over all ranks' loci — the coalescence counts and fixed-point T2h as exact
    integers (two doubles each through the collective), the likelihood + Jacobian sum as a double (summed in rank order here, in
    locus order on one rank: the tolerance below) — and draws the same thetas from the same global stream"""
    one = run(1, str(tmp_path / "one"), 30011, DIST_GTR="1", DIST_PROGRAM="1")[0]
    two = run(2, str(tmp_path / "two"), 30012 + os.getpid() % 500, DIST_GTR="1", DIST_PROGRAM="1")
    assert one["kind"] == "generic" and all(r["kind"] == "generic" for r in two)
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]      # replicated decisions, the same bits
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-9, atol=0) and r["taus"][8:] != [0.001, 0.0012, 0.0025, 0.0011, 0.0013, 0.003, 0.005]
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-9, atol=0) and r["thetas"] != one["thetas"][:0]
    assert one["thetas"][8:] != [0.002]*7 if len(one["thetas"]) >= 15 else True
    times = two[0]["times"] + two[1]["times"]
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert len(times) == len(one["times"])
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=1e-9, atol=0)
    assert np.allclose(lnl, one["lnl"], rtol=1e-9, atol=0)
    assert sum(r["summary"]["accepted"] for r in two) > 0


@pytest.mark.parametrize("shares", ["both", "one"])
def test_two_ranks_with_loci_of_several_kinds(tmp_path, shares):
    """a data set of JC69 loci (persistent-kernel size) and GTR + Gamma4 loci over two ranks (threads.c:234-353 shards any loci,
    method.c:3320-3346 a model per locus): a rank whose share is mixed runs the composite sampler (csrc/composite.hpp) and calls the
    ranks' all-reduce ONCE per all-loci step on its parts' total, so it pairs with a rank whose share is of one kind (`one`: rank 1
    is a plain persistent-kernel sampler in its several-rank form) collective for collective — the single-rank trajectory again"""
    one = run(1, str(tmp_path / "one"), 30211, DIST_COMPOSITE=shares)[0]
    two = run(2, str(tmp_path / "two"), 30212 + os.getpid() % 500, DIST_COMPOSITE=shares)
    assert one["kind"] == "composite" and two[0]["kind"] == "composite"
    assert two[1]["kind"] == ("composite" if shares == "both" else "hybrid")
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]      # replicated decisions
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-10, atol=0) and r["taus"][8:] != [0.001, 0.0012, 0.0025, 0.0011, 0.0013, 0.003, 0.005]
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-10, atol=0)
    times = two[0]["times"] + two[1]["times"]
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert len(times) == len(one["times"]) == 144
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=1e-10, atol=0)
    assert np.allclose(lnl, one["lnl"], rtol=1e-10, atol=0)
    tot = sum(r["summary"]["total_lnl"] for r in two)
    assert abs(tot - one["summary"]["total_lnl"]) < 1e-9 * abs(tot)


@pytest.mark.parametrize("program", [False, True])
def test_two_ranks_exchange_inside_the_persistent_kernel(tmp_path, program):
    """bpa_sampler_set_p2p: both ranks run the persistent iteration kernel for the whole call and exchange the all-loci
    steps' sums inside it, through each other's mailboxes (here: two processes on the one GPU, the mailboxes mapped
    through hipIpc handles) — the single-rank trajectory again.  program: with BPP's kernel and the program's moves (the
    thetas' Gibbs draws and re-draws then come from sums that crossed the mailboxes)"""
    extra = dict(DIST_PROGRAM="1") if program else {}
    one = run(1, str(tmp_path / "one"), 29911, **extra)[0]
    two = run(2, str(tmp_path / "two"), 29912 + os.getpid() % 500, DIST_P2P="1", **extra)
    assert one["kind"] == "persistent" and all(r["kind"] == "persistent" for r in two)
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]
    for r in two:
        assert np.allclose(r["taus"], one["taus"], rtol=1e-10, atol=0) and r["taus"] != [0, 0, 0, 0, 0.001, 0.002, 0.003]
        assert np.allclose(r["thetas"], one["thetas"], rtol=1e-10, atol=0)
    lnl = two[0]["lnl"] + two[1]["lnl"]
    assert np.allclose(lnl, one["lnl"], rtol=1e-10, atol=0)
    times = two[0]["times"] + two[1]["times"]
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=1e-10, atol=0)


@pytest.mark.parametrize("how", ["mailboxes", "callback"])
def test_two_ranks_pool_the_step_length_rule(tmp_path, how):
    """the program's burn-in rule sets ONE step length per move for the whole data set from the acceptance proportions over all
    loci: on two ranks the per-locus moves' counts are pooled first (through the mailboxes' one-shot exchange next to the persistent
    kernel, through the callback on the generic sampler), so both ranks end at the same five step lengths — and those moved"""
    extra = dict(DIST_PROGRAM="1", DIST_BURNIN="1", **(dict(DIST_P2P="1") if how == "mailboxes" else dict(DIST_GTR="1")))
    two = run(2, str(tmp_path / "two"), 30112 + os.getpid() % 500, **extra)
    a, b = two[0]["ft"], two[1]["ft"]
    assert a == b, (a, b)
    start = dict(gage=0.003, gspr=0.005, tau=0.0008, mix=0.2, theta=0.001)
    assert all(a[k] != start[k] for k in ("gage", "gspr", "tau", "mix")), a
    assert two[0]["taus"] == two[1]["taus"] and two[0]["thetas"] == two[1]["thetas"]


# ---- several ranks on one GPU, small shares.  What two ranks cannot show: sums over more than two mailbox slots added in rank
# order, several ranks taking one decision, counts pooled over all of them.  The tests keep the name of BASELINE's eight-GPU world
# size but run MANY = 4 ranks: a shared GPU machine lets at most six processes open a GPU at once, the pytest process among them.
MANY = 4


def _many_against_one(rs, one, rtol):
    assert len(rs) == MANY
    for r in rs:
        assert r["taus"] == rs[0]["taus"] and r["thetas"] == rs[0]["thetas"]               # replicated decisions, the same bits on every rank
        assert np.allclose(r["taus"], one["taus"], rtol=rtol, atol=0) and np.allclose(r["thetas"], one["thetas"], rtol=rtol, atol=0)
    assert [r["first"] for r in rs] == sorted(r["first"] for r in rs) and rs[1]["first"] == len(rs[0]["lnl"])
    times = [t for r in rs for t in r["times"]]
    lnl = [x for r in rs for x in r["lnl"]]
    assert len(times) == len(one["times"])
    for a, b in zip(times, one["times"]):
        assert np.allclose(a, b, rtol=rtol, atol=0)
    assert np.allclose(lnl, one["lnl"], rtol=rtol, atol=0)
    assert one["taus"] != [0, 0, 0, 0, 0.001, 0.002, 0.003]


# Eight PERSISTENT kernels of eight processes exchanging through mailboxes need the one GPU's hardware scheduler to keep all eight
# resident at once; it does not always (round 6, two runs of the same tree: 4.8 s and green / a 43 s time-out in the burn-in test).
# On eight GPUs every kernel has a device to itself.  Those cases run with BPA_TEST_EIGHT_MAILBOXES=1 only; the callback forms
# (host-driven collective between launches: no co-residency condition) always.
EIGHT_MAILBOXES = pytest.mark.skipif(not os.environ.get("BPA_TEST_EIGHT_MAILBOXES"),
                                     reason="eight persistent kernels on ONE GPU: co-residency is the scheduler's choice (set BPA_TEST_EIGHT_MAILBOXES=1)")


@pytest.mark.parametrize("how", ["callback", pytest.param("mailboxes-program", marks=EIGHT_MAILBOXES)])
def test_eight_ranks_walk_the_single_rank_trajectory(tmp_path, how):
    """160 four-taxon loci over MANY ranks: through the all-reduce callback (one collective per all-loci step between
    the launches), through the mailboxes inside the persistent kernel (every control wave adds the slots in rank order), and
    the latter with BPP's moves (fixed-point sums of counts and waiting times from all ranks feed the Gibbs draws)"""
    extra = {}
    if how != "callback":
        extra["DIST_P2P"] = "1"
    if how == "mailboxes-program":
        extra["DIST_PROGRAM"] = "1"
    one_extra = {k: v for k, v in extra.items() if k != "DIST_P2P"}
    one = run(1, str(tmp_path / "one"), 31011, **one_extra)[0]
    rs = run(MANY, str(tmp_path / "many"), 31012 + os.getpid() % 500, **extra)
    assert all(r["kind"] == ("hybrid" if how == "callback" else "persistent") for r in rs), [r["kind"] for r in rs]
    _many_against_one(rs, one, 1e-10 if how != "mailboxes-program" else 1e-9)
    tot = sum(r["summary"]["total_lnl"] for r in rs)
    assert abs(tot - one["summary"]["total_lnl"]) < 1e-9 * abs(tot)


def test_eight_ranks_generic_sampler_with_the_program_s_moves(tmp_path):
    """48 eight-taxon GTR + Gamma4 loci over MANY ranks, BPP's own iteration with the parameter moves: the ranks'
    decision waves (gdec_kernel) take every THETA / TAU / MIX decision from the same all-reduced sums (the integer sums exact, the
    likelihood sum in rank order) — the single rank's chain"""
    one = run(1, str(tmp_path / "one"), 31111, DIST_GTR="1", DIST_PROGRAM="1")[0]
    rs = run(MANY, str(tmp_path / "many"), 31112 + os.getpid() % 500, DIST_GTR="1", DIST_PROGRAM="1")
    assert one["kind"] == "generic" and all(r["kind"] == "generic" for r in rs)
    _many_against_one(rs, one, 1e-9)
    assert sum(r["summary"]["accepted"] for r in rs) > 0


@EIGHT_MAILBOXES
def test_eight_ranks_pool_the_step_length_rule(tmp_path):
    """the burn-in rule over MANY ranks' mailboxes: the per-locus moves' counts of all shares pooled in one exchange, every
    rank ends at the same five step lengths"""
    rs = run(MANY, str(tmp_path / "many"), 31212 + os.getpid() % 500, DIST_PROGRAM="1", DIST_BURNIN="1", DIST_P2P="1")
    assert all(r["ft"] == rs[0]["ft"] for r in rs), [r["ft"] for r in rs]
    start = dict(gage=0.003, gspr=0.005, tau=0.0008, mix=0.2, theta=0.001)
    assert all(rs[0]["ft"][k] != start[k] for k in ("gage", "gspr", "tau", "mix")), rs[0]["ft"]
    assert all(r["taus"] == rs[0]["taus"] and r["thetas"] == rs[0]["thetas"] for r in rs)
