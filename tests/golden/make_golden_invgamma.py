"""Posterior of the UNMODIFIED reference program (oracle/_ref/bpp, A00, JC69) under its DEFAULT priors, the inverse gammas
`thetaprior = invgamma a b e` and `tauprior = invgamma a b` (cfile.c:1550, 1641; bpp.c:644-647), on the synthetic 20-locus
4-species data set of make_golden_heredity.py: the known answer for the samplers' inverse-gamma forms of THETA (window and
the exact Gibbs draw, stree.c:3698-3707, 3822), TAU (stree.c:5667, 5930-5989) and MIX (prop_mixing.c:366-423, 502-507)
(tests/test_invgamma_host.py, tests/test_gpu_invgamma.py).

    python tests/golden/make_golden_invgamma.py     ->  tests/golden/invgamma_posterior.json

The data recipe and the run length are make_golden_heredity.py's: bpp_amd.synth (seed 91; the tests regenerate the data), a
sequential PHYLIP file + Imap + control file, 3 000 burn-in + 12 000 x 2 iterations — TWICE, with seeds 1 and 2.  a = 3 on
both priors; b puts each prior's mean b/(a - 1) at the value the data were simulated with (theta 0.004, root tau 0.003).  `e`
keeps the thetas in the chain (without it the program integrates them out and prints no theta column): the generator asserts
that out.mcmc.txt carries the theta columns.  Seed 1's summary (mean and sd of every theta, every tau, lnL) is `posterior`,
seed 2's `posterior_seed2`; the generator asserts that seed 2 lies within the tests' own bars of seed 1 (0.3 sd on the means,
0.25 sd on the sds).  Only the summaries go into the fixture.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from bpp_amd import synth          # noqa: E402

CFG = dict(nloci=20, sites=500, taxa=4, seed=91, theta=0.004, theta_prior=(3.0, 0.008), tau_prior=(3.0, 0.006),
           burnin=3000, sampfreq=2, nsample=12000, seeds=(1, 2), tol_mean=0.3, tol_sd=0.25)


def run(data, seed):
    names = "ABCD"
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "seqs.txt"), "w") as f:
            for d in data:
                seqs = ["".join(ch * int(w) for ch, w in zip(s, d["weights"])) for s in d["seqs"]]
                f.write(f"4 {len(seqs[0])}\n")
                for nm, s in zip(names, seqs):
                    f.write(f"s^{nm.lower()}  {s}\n")
                f.write("\n")
        with open(os.path.join(td, "imap.txt"), "w") as f:
            f.write("".join(f"{c.lower()} {c}\n" for c in names))
        with open(os.path.join(td, "a00.ctl"), "w") as f:
            f.write(f"seed = {seed}\nseqfile = seqs.txt\nImapfile = imap.txt\njobname = out\nspeciesdelimitation = 0\n"
                    "speciestree = 0\nspecies&tree = 4  A B C D\n                  1 1 1 1\n"
                    "                 (((A, B), C), D);\nusedata = 1\n"
                    f"nloci = {CFG['nloci']}\nmodel = jc69\ncleandata = 0\n"
                    f"thetaprior = invgamma {CFG['theta_prior'][0]:g} {CFG['theta_prior'][1]:g} e\n"
                    f"tauprior = invgamma {CFG['tau_prior'][0]:g} {CFG['tau_prior'][1]:g}\nfinetune = 1\nprint = 1 0 0 0\n"
                    f"burnin = {CFG['burnin']}\nsampfreq = {CFG['sampfreq']}\nnsample = {CFG['nsample']}\n")
        subprocess.run([os.path.join(ROOT, "oracle", "_ref", "bpp"), "--cfile", "a00.ctl"], cwd=td, check=True,
                       stdout=subprocess.DEVNULL)
        rows = [ln.split("\t") for ln in open(os.path.join(td, "out.mcmc.txt"))]
    head = [h.strip() for h in rows[0]]
    body = np.array([[float(x) for x in r] for r in rows[1:]])
    return head, len(body), {h: dict(mean=float(body[:, c].mean()), sd=float(body[:, c].std())) for c, h in enumerate(head) if c > 0}


def main():
    _, tau, _ = synth.species_tree_arrays(CFG["taxa"], CFG["theta"])
    a, b = CFG["theta_prior"]
    assert abs(b/(a - 1) - CFG["theta"]) < 1e-15 and abs(CFG["tau_prior"][1]/(CFG["tau_prior"][0] - 1) - tau[-1]) < 1e-15
    data = synth.make_dataset(CFG["nloci"], CFG["sites"], CFG["taxa"], "jc69", 1, seed=CFG["seed"], theta=CFG["theta"])
    head, n, post = run(data, CFG["seeds"][0])
    _, n2, post2 = run(data, CFG["seeds"][1])
    thetas = [h for h in head if h.startswith("theta:")]
    assert len(thetas) == 3 and len([h for h in head if h.startswith("tau:")]) == 3 and "lnL" in head, head
    assert n == n2 == CFG["nsample"]
    worst = dict(mean=0.0, sd=0.0)
    for name, ref in post.items():
        dm, ds = abs(post2[name]["mean"] - ref["mean"])/ref["sd"], abs(post2[name]["sd"] - ref["sd"])/ref["sd"]
        worst["mean"], worst["sd"] = max(worst["mean"], dm), max(worst["sd"], ds)
        assert dm < CFG["tol_mean"] and ds < CFG["tol_sd"], (name, ref, post2[name])
    out = dict(config=dict(CFG), columns=head, samples=n, seed2_worst=worst, posterior=post, posterior_seed2=post2)
    print(json.dumps(post, indent=1))
    print("seed 2 against seed 1, worst differences in sd units:", worst)
    with open(os.path.join(HERE, "invgamma_posterior.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
