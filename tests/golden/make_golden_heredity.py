"""Posterior of the UNMODIFIED reference program (oracle/_ref/bpp, A00, JC69) with heredity scalars, in both forms the
control file offers, on a synthetic 20-locus 4-species data set: the known answer for the samplers' heredity scalars in the MSC
density, in the THETA / TAU / MIX sums and for the HRDT move (gtree_update_logprob_contrib gtree.c:3859, prop_heredity
gtree.c:8214) next to their tree moves (tests/test_heredity_posterior.py).

    python tests/golden/make_golden_heredity.py     ->  tests/golden/heredity_posterior.json

  estimated  `heredity = 1 4 4`: h_i ~ gamma(4, 4), moved by the program's own move;
  fixed      `heredity = 2 <file>`: the 20 loci cycle through 1.0 / 0.75 / 0.25 (autosomal, X-linked, mitochondrial).

The data recipe, priors and run length are make_golden_locusrate.py's: bpp_amd.synth (seed 91; the tests regenerate the
data), a sequential PHYLIP file + Imap + control file, 3 000 burn-in + 12 000 x 2 iterations, thetaprior = gamma 2 500,
tauprior = gamma 2 300 — each form TWICE, with seeds 1 and 2.  Seed 1's summary (mean and sd of every theta, every tau, lnL)
is the form's `posterior`, seed 2's its `posterior_seed2`; the generator asserts that seed 2 lies within the tests' own bars
of seed 1 (0.3 sd on the means, 0.25 sd on the sds) — a fixture the program itself cannot reproduce from another seed would
test nothing.  Only the summaries go into the fixture.
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

CFG = dict(nloci=20, sites=500, taxa=4, seed=91, theta=0.004, theta_prior=(2.0, 500.0), tau_prior=(2.0, 300.0),
           heredity_prior=(4.0, 4.0), heredity_fixed=(1.0, 0.75, 0.25), burnin=3000, sampfreq=2, nsample=12000, seeds=(1, 2), tol_mean=0.3, tol_sd=0.25)


def run(data, seed, form):
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
        if form == "estimated":
            line = "heredity = 1 %g %g" % CFG["heredity_prior"]
        else:
            with open(os.path.join(td, "heredity.txt"), "w") as f:
                f.write(" ".join("%g" % CFG["heredity_fixed"][i % 3] for i in range(CFG["nloci"])) + "\n")
            line = "heredity = 2 heredity.txt"
        with open(os.path.join(td, "a00.ctl"), "w") as f:
            f.write(f"seed = {seed}\nseqfile = seqs.txt\nImapfile = imap.txt\njobname = out\nspeciesdelimitation = 0\n"
                    "speciestree = 0\nspecies&tree = 4  A B C D\n                  1 1 1 1\n"
                    "                 (((A, B), C), D);\nusedata = 1\n"
                    f"nloci = {CFG['nloci']}\nmodel = jc69\ncleandata = 0\n"
                    f"{line}\n"
                    f"thetaprior = gamma {CFG['theta_prior'][0]:g} {CFG['theta_prior'][1]:g}\n"
                    f"tauprior = gamma {CFG['tau_prior'][0]:g} {CFG['tau_prior'][1]:g}\nfinetune = 1\nprint = 1 0 0 0\n"
                    f"burnin = {CFG['burnin']}\nsampfreq = {CFG['sampfreq']}\nnsample = {CFG['nsample']}\n")
        subprocess.run([os.path.join(ROOT, "oracle", "_ref", "bpp"), "--cfile", "a00.ctl"], cwd=td, check=True,
                       stdout=subprocess.DEVNULL)
        rows = [ln.split("\t") for ln in open(os.path.join(td, "out.mcmc.txt"))]
    head = [h.strip() for h in rows[0]]
    body = np.array([[float(x) for x in r] for r in rows[1:]])
    return head, len(body), {h: dict(mean=float(body[:, c].mean()), sd=float(body[:, c].std())) for c, h in enumerate(head) if c > 0}


def main():
    data = synth.make_dataset(CFG["nloci"], CFG["sites"], CFG["taxa"], "jc69", 1, seed=CFG["seed"], theta=CFG["theta"])
    out = dict(config=dict(CFG))
    for form in ("estimated", "fixed"):
        head, n, post = run(data, CFG["seeds"][0], form)
        _, n2, post2 = run(data, CFG["seeds"][1], form)
        worst = dict(mean=0.0, sd=0.0)
        for name, ref in post.items():
            dm, ds = abs(post2[name]["mean"] - ref["mean"])/ref["sd"], abs(post2[name]["sd"] - ref["sd"])/ref["sd"]
            worst["mean"], worst["sd"] = max(worst["mean"], dm), max(worst["sd"], ds)
            assert dm < CFG["tol_mean"] and ds < CFG["tol_sd"], (form, name, ref, post2[name])
        out[form] = dict(columns=head, samples=n, seed2_worst=worst, posterior=post, posterior_seed2=post2)
        print(form, json.dumps(post, indent=1))
        print(form, "seed 2 against seed 1, worst differences in sd units:", worst)
    with open(os.path.join(HERE, "heredity_posterior.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
