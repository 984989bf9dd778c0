/*
 * bpp_amd_priors.h — the prior families of the thetas and of the root tau, and every expression of the THETA / TAU / MIX
 * decisions that depends on the family.  Part of bpp_amd_host.h (which includes it after the pieces these build on); A00_HD
 * functions: they compile for the host driver and for the device decisions alike.
 */
#ifndef BPP_AMD_PRIORS_H
#define BPP_AMD_PRIORS_H

/* ---- the two prior families of the thetas and of the root tau: BPP's 'thetaprior = gamma a b' / 'tauprior = gamma a b'
   (kind 0, the expressions the driver always had, unchanged to the bit) and its DEFAULT, the inverse gamma of
   'thetaprior = invgamma a b e' / 'tauprior = invgamma a b' (kind 1; cfile.c:1550, bpp.c:644-647).  One statement of every
   expression for the host driver and the device decisions (a00_set_prior_kinds, bpa_sampler_set_prior_kinds).
     theta prior ratio   (-a - 1) log(t'/t) - b (1/t' - 1/t)                            stree.c:3865, 5701, 5987; prop_mixing.c:422
     root tau, TAU       (-a - 1 - (S-1) + 1) log(t'/t) - b (1/t' - 1/t)                 stree.c:5667 (candidate_count = S - 1)
     root tau, MIX       (-a - 1) log c - b (1/t' - 1/t) - (S-2) log c                   prop_mixing.c:502-507 (tau_count = S - 1:
                         the inner populations, prop_mixing.c:297-308; written as the gamma branch is, the Dirichlet part beside
                         the root's own term)
     theta's conditional given the gene trees is EXACTLY inverse-gamma(a + k, b + T): no fit, no special case for T = 0 (k = 0,
                         T = 0: the prior); the Gibbs draw b1 / gamma(a1) of THETA is accepted without an acceptance number
                         (stree.c:3698-3707, 3822); the re-draws of TAU and MIX enter with a00_invgamma_logpdf as before
                         (stree.c:5930-5989, prop_mixing.c:366-423)                                                          */
#define A00_PRIOR_GAMMA    0
#define A00_PRIOR_INVGAMMA 1
static inline A00_HD double a00_theta_prior_lnratio(int kind, double a, double b, double told, double tnew)
{
  if (kind == A00_PRIOR_INVGAMMA) return (-a - 1)*log(tnew/told) - b*(1/tnew - 1/told);
  return (a - 1)*log(tnew/told) - b*(tnew - told);
}
static inline A00_HD double a00_tau_prior_lnratio(int kind, double a, double b, int S, double told, double tnew)
{
  if (kind == A00_PRIOR_INVGAMMA) return (-a - 1 - (S - 1) + 1)*log(tnew/told) - b*(1/tnew - 1/told);
  return (a - 1 - (S - 1) + 1)*log(tnew/told) - b*(tnew - told);
}
static inline A00_HD double a00_mix_tau_prior_lnratio(int kind, double a, double b, int S, double lnc, double told, double tnew)
{
  if (kind == A00_PRIOR_INVGAMMA) return (-a - 1)*lnc - b*(1/tnew - 1/told) - (double)(S - 2)*lnc;
  return (a - 1)*lnc - b*(tnew - told) - (double)(S - 2)*lnc;
}
/* the inverse gamma theta' = b1 / gamma(a1) is drawn from: the fit above for a gamma prior, the conditional itself otherwise */
static inline A00_HD void a00_theta_conditional_kind(int kind, double a, double b, long k, double T, double * a1, double * b1)
{
  if (kind == A00_PRIOR_INVGAMMA) { *a1 = a + k; *b1 = b + T; return; }
  a00_theta_conditional_invgamma(a, b, k, T, a1, b1);
}
/* a00_theta_lnacc with the prior's kind */
static inline A00_HD double a00_theta_lnacc_kind(int kind, long k, double T, double told, double tnew, double a, double b)
{
  if (kind == A00_PRIOR_INVGAMMA)
    return (k*(log(2.0/tnew) - log(2.0/told)) - (T/tnew - T/told)) + a00_theta_prior_lnratio(kind, a, b, told, tnew);
  return a00_theta_lnacc(k, T, told, tnew, a, b);
}

/* ---- the substitution-parameter moves by model (a00_set_subst_kind; the device samplers read the locus's own model).
   `model` is BPA_DNA_MODEL_* (bpp_amd.h: 0 JC69, 1 K80, 2 F81, 3 HKY, 4 T92, 5 TN93, 6 F84, 7 GTR; anything above, the
   device's 100 for "eigendecomposition" included, moves as GTR).  One statement for the host driver and the device kernels.
     exchangeability entries   K80, HKY, T92, F84: 2   TN93: 3   GTR: 6   JC69, F81: none          locus.c:906-952
     their reference entry     TN93: 2   every other model: 1 (GTR: the A<->G rate)               locus.c:3197-3229
     frequencies               JC69, K80: none   every other model: 0, 1, 2 against T (entry 3)   locus.c:2782-2791
   Step s of a kind proposes the locus's s-th moving entry (GTR: 0, 2, 3, 4, 5 — the order the moves always had); a locus
   whose model has fewer sits the step out.                                                                                 */
static inline A00_HD int a00_subst_qrates(int model)
{
  return model >= 7 ? 6 : model == 5 ? 3 : (model == 0 || model == 2) ? 0 : 2;
}
static inline A00_HD int a00_subst_ref(int which /* 1 frequencies, 2 exchangeabilities */, int model)
{
  return which == 1 ? 3 : model == 5 ? 2 : 1;
}
static inline A00_HD int a00_subst_steps(int which, int model)
{
  if (which == 1) return (model == 0 || model == 1) ? 0 : 3;
  return a00_subst_qrates(model) > 0 ? a00_subst_qrates(model) - 1 : 0;
}
/* the entry step s moves, -1: this model has no such step */
static inline A00_HD int a00_subst_entry(int which, int model, int s)
{
  if (s < 0 || s >= a00_subst_steps(which, model)) return -1;
  return (which == 2 && s >= a00_subst_ref(2, model)) ? s + 1 : s;
}
/* the Dirichlet(a) prior on a model's exchangeabilities in the move of entry j against the reference entry: what joins
   (log q_j' - log q_j) in the Hastings term,
     (a_j - 1)(log q_j' - log q_j) + (a_ref - 1) log(q_ref'/q_ref)                              locus.c:3190, 3301-3304
   for every model, indexed by j and ref; the program's a is {2,4,2,2,4,2}.  A term whose a is 1 is not formed (as in the
   reference), so a prior of ones leaves the Hastings term what it was, to the bit.                                        */
static inline A00_HD double a00_qrates_prior_lnratio(const double * a, int j, int ref, double lj_old, double lj_new, double ref_old, double ref_new)
{
  double r = 0;
  if (a[j] - 1 != 0) r += (a[j] - 1.0)*(lj_new - lj_old);
  if (a[ref] - 1 != 0) r += (a[ref] - 1.0)*log(ref_new/ref_old);
  return r;
}
static inline A00_HD int a00_qrates_prior_flat(const double * a)
{
  int q, flat = 1;
  for (q = 0; q < 6; ++q) flat = flat && a[q] == 1.0;
  return flat;
}

#endif
