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

#endif
