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

/* ---- the program's THETA / TAU / MIX decisions on the host, "from the sums" (a00_set_program_moves): ONE statement for the
   host driver (a00_driver.c: theta_step_gibbs, tau_step, mix_step) and the generic sampler's host_decisions form
   (gsampler_host.hpp: gs_prog_*) — one order of draws from the global stream and of floating-point operations, which is what
   the two walk one trajectory by.  Host only (plain C, no A00_HD); the callers keep their sums, counters and decision logs.  */
#define A00_FX40     1099511627776.0                  /* the sums of T2h/h are sums of 2^-40 fixed-point terms: no order */
#define A00_FX40_INV (1.0/1099511627776.0)
/* BPP's acceptance rule on a legacy_rndu state: the number is drawn only when needed (gtree.c:5476, stree.c:6286) */
static inline int a00_bpp_accept(unsigned int * z, double lnacc) { return lnacc >= -1e-10 || a00_bpp_rndu(z) < exp(lnacc); }
/* the caller's arrays for the length of one step (a view: nothing is owned, nothing a kernel reads) */
typedef struct a00_prog
{
  int npop; unsigned has;                 /* bit p: population p has a theta */
  int kind; double a, b;                  /* the thetas' prior */
  long long * k; double * T; int ok;      /* k_p, T_p of the current trees, carried from THETA's sums on; ok = 0: unusable */
  double * theta; unsigned int * z;       /* z: the global stream */
} a00_prog_t;
/* ONE theta re-drawn inside TAU or MIX: theta' = b1/gamma(a1) from the inverse gamma fitted to its conditional given
   (k, T_new); returns its term of the acceptance ratio: proposal ratio (the old conditional fitted to T_fit_old), prior ratio,
   the densities' change over all loci k (log 2/theta' - log 2/theta) - (T_new/theta' - T_old/theta).  TAU: T_fit_old = T_old;
   MIX: T_fit_old = (c T)/c, T_old = T — not always the same bits.  NaN where either fit is NaN: then nothing is drawn.   */
static inline double a00_prog_redraw_theta(const a00_prog_t * g, long k, double T_fit_old, double T_old, double T_new, double to, double * tn)
{
  double a1, b1, a1o, b1o, t;
  a00_theta_conditional_kind(g->kind, g->a, g->b, k, T_new, &a1, &b1);
  a00_theta_conditional_kind(g->kind, g->a, g->b, k, T_fit_old, &a1o, &b1o);
  if (!(a1 == a1 && a1o == a1o)) return NAN;
  *tn = t = 1.0/(a00_bpp_rndgamma(g->z, a1)/b1);
  return (a00_invgamma_logpdf(to, a1o, b1o) - a00_invgamma_logpdf(t, a1, b1))
       + a00_theta_prior_lnratio(g->kind, g->a, g->b, to, t)
       + (k*(log(2.0/t) - log(2.0/to)) - (T_new/t - T_old/to));
}
/* THETA, first half — before the sums exist: per population in order, "slide or Gibbs" and the window of the sliding ones */
static inline void a00_prog_theta_propose(const a00_prog_t * g, double slide_prob, double ft_theta, int * slide, double * tnew)
{
  int p;
  for (p = 0; p < g->npop; ++p)
  {
    slide[p] = 0; tnew[p] = g->theta[p];
    if (!(g->has >> p & 1u)) continue;
    slide[p] = a00_bpp_rndu(g->z) < slide_prob;
    if (slide[p]) tnew[p] = a00_reflect(g->theta[p] + ft_theta*a00_bpp_rnd_symmetrical(g->z), 0.0, 999.0);
  }
}
/* THETA, second half — k, T, ok are the sums': the Gibbs variates of all populations first (the device takes them side by
   side), then per population the ratio and the decision; an inverse-gamma prior's Gibbs draw is the conditional's own: accepted,
   no acceptance number (stree.c:3822).  Accepted thetas are stored; lnacc[] (NaN: unusable sums, failed fit) is for the logs */
static inline void a00_prog_theta_decide(const a00_prog_t * g, const int * slide, double * tnew, int * acc, double * lnacc)
{
  double fa[A00_MAXPOP], fb[A00_MAXPOP]; int p;
  for (p = 0; p < g->npop; ++p)
  {
    fa[p] = fb[p] = NAN;
    if (!(g->has >> p & 1u) || !g->ok || slide[p]) continue;
    a00_theta_conditional_kind(g->kind, g->a, g->b, (long)g->k[p], g->T[p], &fa[p], &fb[p]);
    if (fa[p] == fa[p]) tnew[p] = 1/(a00_bpp_rndgamma(g->z, fa[p])/fb[p]);
  }
  for (p = 0; p < g->npop; ++p)
  {
    const long k = (long)g->k[p]; const double T = g->T[p], to = g->theta[p];
    lnacc[p] = NAN; acc[p] = 0;
    if (!(g->has >> p & 1u) || !g->ok) continue;
    if (slide[p]) lnacc[p] = a00_theta_lnacc_kind(g->kind, k, T, to, tnew[p], g->a, g->b);
    else if (fa[p] == fa[p] && g->kind == A00_PRIOR_INVGAMMA) lnacc[p] = tnew[p] == tnew[p] ? 0.0 : NAN;
    else if (fa[p] == fa[p]) lnacc[p] = a00_theta_lnacc(k, T, to, tnew[p], g->a, g->b) + a00_theta_gibbs_hastings(fa[p], fb[p], to, tnew[p]);
    acc[p] = lnacc[p] == lnacc[p] && tnew[p] > 0 && a00_bpp_accept(g->z, lnacc[p]);
    if (acc[p]) g->theta[p] = tnew[p];
  }
}
/* TAU of population aff[0] with its children aff[1], aff[2]: `sum` is the loci's part with the root's prior term, c[] the
   three populations' new fixed-point sums (-> Cn[], their T after the move; usable = 0: a term was out of range); re-draws
   the three thetas (oldtheta[] keeps them for a rejection) and returns the acceptance ratio, NaN on unusable sums or a failed fit */
static inline double a00_prog_tau_lnacc(const a00_prog_t * g, const int * aff, const long long * c, int usable, double sum, double * Cn, double * oldtheta)
{
  int j;
  for (j = 0; j < 3; ++j)
  {
    const int p = aff[j]; double tn, add;
    oldtheta[j] = g->theta[p]; Cn[j] = (double)c[j]*A00_FX40_INV;
    if (!(g->has >> p & 1u)) continue;
    if (!usable || !g->ok) { sum = NAN; continue; }
    add = a00_prog_redraw_theta(g, (long)g->k[p], g->T[p], g->T[p], Cn[j], oldtheta[j], &tn);
    if (add != add) { sum = NAN; continue; }
    sum += add; g->theta[p] = tn;
  }
  return sum;
}
/* MIX, before the loci are proposed: every theta from its conditional given the scaled trees (k, c T), in population order
   (prop_mixing.c:272-425); oldtheta[] keeps all of them; returns the thetas' part of the acceptance ratio */
static inline double a00_prog_mix_thetas(const a00_prog_t * g, double c, double * oldtheta)
{
  double lnacc_theta = 0; int p;
  for (p = 0; p < g->npop; ++p) oldtheta[p] = g->theta[p];
  for (p = 0; p < g->npop; ++p)
  {
    double Ts, tn, add;
    if (!(g->has >> p & 1u)) continue;
    if (!g->ok) { lnacc_theta = NAN; continue; }
    Ts = g->T[p]*c;
    add = a00_prog_redraw_theta(g, (long)g->k[p], Ts/c, g->T[p], Ts, oldtheta[p], &tn);
    if (add != add) { lnacc_theta = NAN; continue; }
    lnacc_theta += add; g->theta[p] = tn;
  }
  return lnacc_theta;
}
/* MIX's ratio from the loci's sum: (S - 1) log c, the root tau's prior (the Dirichlet part is unchanged), the thetas' part */
static inline double a00_mix_lnacc(double sum, int S, double lnc, int tau_kind, double tau_a, double tau_b, double root_old, double root_new, double lnacc_theta)
{
  double lnacc = sum + (double)(S - 1)*lnc;
  if (tau_a > 0) lnacc += a00_mix_tau_prior_lnratio(tau_kind, tau_a, tau_b, S, lnc, root_old, root_new);
  return lnacc + lnacc_theta;
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
