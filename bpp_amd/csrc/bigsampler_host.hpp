// bigsampler_host.hpp — host side of the big-tree device sampler (bigsampler.hpp), what is its own: the upload, one step launch
// (gb_step), one evaluation (gb_eval), the head of the download.  The launch loop of an iteration is the generic sampler's
// (gsampler_host.hpp: gs_iterate), which reaches the two launches through sampler_step / sampler_eval, defined below.
// Included at the end of sampler.hpp, after gsampler_host.hpp (whose buffers and all-loci kernels it shares).
#pragma once

// the substitution-parameter moves' tables (gs_subst_ready: the generic sampler's, with its refusals) and the loci's bytes for
// big_par_kernel, made when a window width first becomes positive: a sampler that never set one has none of them
static int gb_subst_ready(bpa_sampler * s)
{
  if (!gs_subst_ready(s)) return 0;
  if (!s->g_sm.p || s->b_par_todo.p) return 1;
  if (!s->b_par_todo.reserve(s->nloci)) return 0;
  HIPCHK(hipMemsetAsync(s->b_par_todo.p, 0, s->nloci, s->eng->stream));
  return 1;
}

static int gb_upload(bpa_sampler * s)
{
  bpa_engine * e = s->eng;
  const unsigned T = s->nloci;
  if (!flush_state(e)) return 0;                    // (tip states, weights, parameter blocks, eigensystems on the device)
  for (unsigned i = 0; i < T; ++i)
  {
    gbig::BTree & t = s->b_trees[i];
    if (!assign_pops_host(s, t)) return 0;
    // the scaler that goes with an inner node's CURRENT CLV buffer (gtree.c:2433-2439 at the start: its index among the
    // inner nodes; swap_clv toggles the two together, so scaler = clv - tips holds in mid-run too)
    for (int k = 0; k < 2*t.tips - 1; ++k) t.scaler[k] = (int16_t)((s->loci[i]->scale_buffers && k >= t.tips) ? t.clv[k] - t.tips : BPA_SCALE_BUFFER_NONE);
    for (int p = 0; p < smp::MAXPOP; ++p) t.gl[p] = 0;
    for (int k = 0; k < t.tips; ++k) for (int q = t.pop[k]; q >= 0; q = s->sp.parent[q]) t.gl[q]++;
  }
  for (int p = 0; p < smp::MAXPOP; ++p) s->has_theta[p] = p >= s->sp.S && p < s->sp.npop;
  std::vector<uint32_t> tl(T), tp(T + 1), thr;
  unsigned off = 0;
  for (unsigned i = 0; i < T; ++i)
  {
    const gbig::BTree & t = s->b_trees[i];
    int cnt[smp::MAXPOP] = {0};
    for (int k = 0; k < t.tips; ++k) if (++cnt[t.pop[k]] >= 2) s->has_theta[t.pop[k]] = true;
    tl[i] = s->loci[i]->id; tp[i] = off; off += s->loci[i]->sites;
    for (unsigned n = 0; n < s->loci[i]->sites; ++n) thr.push_back(i);
  }
  tp[T] = off;
  s->g_npat = off;
  s->g_maxmat = 2*s->maxtips - 2; s->g_maxops = s->maxtips - 1;
  const size_t nmat = (size_t)T*s->g_maxmat;
  uint32_t zero2[2] = {0, 0};
  if (!upload(s->b_dev, s->b_trees.data(), T) || !s->b_undo.reserve(T) || !upload(s->g_tlocus, tl.data(), T) || !upload(s->g_tpat, tp.data(), T + 1) ||
      !upload(s->b_thr, thr.data(), thr.size()) || !s->g_rscaler.reserve(T) || !s->g_ops20.reserve((size_t)T*s->g_maxops) ||
      !s->g_oprng.reserve((size_t)2*T) || !s->g_root20.reserve(T) || !s->g_mtask.reserve(nmat) || !s->g_mpm.reserve(nmat) || !s->g_len.reserve(nmat) ||
      !s->g_lnl.reserve(T) || !s->g_lnlcur.reserve(T) || !s->g_hast.reserve(T) || !s->g_logpr.reserve(T) || !s->g_delta.reserve(T) || !s->g_active.reserve(T) ||
      !s->g_site.reserve(off) || !upload(s->flag, zero2, 1) || !upload(s->counters, s->h_counters, 4) || !s->mix_sum.reserve(1) ||
      !upload(s->taus, s->h_taus.data(), s->h_taus.size()) || !s->pop_t2h.reserve((size_t)T*smp::MAXPOP) ||
      !s->pop_nc.reserve((size_t)T*smp::MAXPOP) || !s->theta_sums.reserve(smp::MAXPOP))
    return 0;
  HIPCHK(hipMemsetAsync(s->g_oprng.p, 0, (size_t)2*T*sizeof(uint32_t), e->stream));
  HIPCHK(hipMemsetAsync(s->g_root20.p, 0, (size_t)T*sizeof(uint32_t), e->stream));
  HIPCHK(hipMemsetAsync(s->g_rscaler.p, 0xff, (size_t)T*sizeof(int32_t), e->stream));
  HIPCHK(hipMemsetAsync(s->g_mtask.p, 0xff, nmat*sizeof(uint32_t), e->stream));
  HIPCHK(hipMemsetAsync(s->g_mpm.p, 0, nmat*sizeof(uint32_t), e->stream));
  HIPCHK(hipMemsetAsync(s->g_len.p, 0, nmat*sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->g_lnl.p, 0, T*sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->g_hast.p, 0, T*sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->g_logpr.p, 0, T*sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->g_delta.p, 0, T*sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->g_active.p, 0, T, e->stream));
  if (s->allreduce) return fail("bpa_sampler: the big-tree sampler runs on one rank (a handful of loci: nothing to shard)");
  // the rates' and the scalars' arrays where some were set or a move is on (gs_lr_ready / gs_hered_ready: the generic sampler's)
  s->g_mui.free(); s->g_mui_old.free(); s->g_lr.free(); s->g_hered.free();
  if (!gs_lr_ready(s) || !gs_hered_ready(s)) return 0;
  // ... and the substitution parameters' (re-made from the host copy, as gs_upload does)
  s->g_sm.free(); s->b_par_todo.free();
  if (!gb_subst_ready(s)) return 0;
  s->epoch = 0; s->mix_pending = false; s->g_pend = 0; s->g_pend_mode = 0; s->g_pend_k = 0;
  s->uploaded = true; s->gp_mirror = false;           // (the program's moves: the decisions' state goes to the device again, gs_prog_ready)
  return 1;
}

// one big_step_kernel launch: settle what is pending, then propose `mode`
static int gb_step(bpa_sampler * s, unsigned mode, unsigned k = 0, double tau_u = 0, double mix_c = 1.0, double mix_lnc = 0)
{
  bpa_engine * e = s->eng;
  gbig::BArgs a{};
  a.trees = s->b_dev.p; a.undo = s->b_undo.p; a.T = s->nloci; a.mode = mode; a.k = k;
  a.pend = s->g_pend; a.pend_mode = s->g_pend_mode; a.lnl_new = s->g_lnl.p; a.hast = s->g_hast.p; a.logpr_new = s->g_logpr.p; a.delta = s->g_delta.p;
  a.active = s->g_active.p; a.flag = s->flag.p; a.epoch = s->epoch; a.lnl_cur = s->g_lnlcur.p;
  a.ops = s->g_ops20.p; a.op_rng = s->g_oprng.p; a.root_clv = s->g_root20.p; a.root_scaler = s->g_rscaler.p;
  a.mat_task = s->g_mtask.p; a.mat_pm = s->g_mpm.p; a.mat_length = s->g_len.p; a.maxmat = s->g_maxmat; a.maxops = s->g_maxops;
  a.taus = s->taus.p; a.tau_q = k; a.tau_u = tau_u; a.mix_c = mix_c; a.mix_lnc = mix_lnc;
  a.pop_nc = s->pop_nc.p; a.pop_t2h = s->pop_t2h.p;
  a.refresh_logpr = s->logpr_stale ? 1u : 0u; s->logpr_stale = false;
  a.prog = gs_prog(s) ? 1u : 0u; a.dstep = s->g_dst.p; a.t2h3 = s->g_t2h3.p;
  a.mui = s->g_mui.p; a.mui_old = s->g_mui_old.p; a.lr = s->g_lr.p; a.ft_mui = s->g_lr_ft[0]; a.a_mui = s->g_a_mui;
  a.hered = s->g_hered.p; a.ft_h = s->g_h_ft; a.h_a = s->g_h_a; a.h_b = s->g_h_b;
  if (mode == 9 && !a.mui) return fail("bpa_sampler: a rate step without the rates' arrays");
  if (mode == 10 && !a.hered) return fail("bpa_sampler: a heredity step without the scalars' array");
  a.sm = s->g_sm.p; a.sm_old = s->g_sm_old.p; a.pend_k = s->g_pend_k; a.par_todo = s->b_par_todo.p; a.loci = e->d_loci.p; a.ids = s->g_ids.p;
  a.ft_freqs = s->g_ft[0]; a.ft_qrates = s->g_ft[1]; a.ft_alpha = s->g_ft[2]; a.alpha_a = s->g_alpha_a; a.alpha_b = s->g_alpha_b;
  for (int q = 0; q < 6; ++q) a.qprior[q] = s->g_qprior[q];
  a.qprior_on = s->g_qprior_on ? 1u : 0u;
  const bool par_step = mode >= 6 && mode <= 8, par_settled = s->g_pend == 4 && s->g_pend_mode >= 6 && s->g_pend_mode <= 8;
  if ((par_step || par_settled) && !(a.sm && a.par_todo)) return fail("bpa_sampler: a substitution-parameter step without the moves' tables");
  a.sp = s->sp;
  // one workgroup per locus; BPP's proposal kernel is the other instantiation; a launch that proposes a substitution parameter
  // or settles such a step takes the instantiation that carries the moves' code (every other launch: the code without it)
  if (par_step || par_settled)
  {
    if (s->kernel_bpp) hipLaunchKernelGGL((gbig::big_step_kernel<true, true>), dim3(s->nloci), dim3(gbig::BBS), 0, e->stream, a);
    else hipLaunchKernelGGL((gbig::big_step_kernel<false, true>), dim3(s->nloci), dim3(gbig::BBS), 0, e->stream, a);
  }
  else if (s->kernel_bpp) hipLaunchKernelGGL((gbig::big_step_kernel<true>), dim3(s->nloci), dim3(gbig::BBS), 0, e->stream, a);
  else hipLaunchKernelGGL((gbig::big_step_kernel<false>), dim3(s->nloci), dim3(gbig::BBS), 0, e->stream, a);
  HIPCHK(hipGetLastError());
  s->launches++;
  // a launch that proposed a substitution parameter, or settled such a step (its rejections put old values back): the loci's
  // parameter blocks and eigensystems follow the sampler's copy before anything — this step's P-matrices, a later evaluation,
  // a download — reads them.  Loci whose byte is clear cost the launch nothing but their workgroup
  if (par_step || par_settled)
  {
    hipLaunchKernelGGL(gbig::big_par_kernel, dim3(s->nloci), dim3(gbig::BBS), 0, e->stream, s->b_par_todo.p, (const double *)s->g_sm.p,
                       (const LocusDev *)e->d_loci.p, (const uint32_t *)s->g_ids.p, (uint32_t)s->nloci);
    HIPCHK(hipGetLastError());
    s->launches++;
  }
  s->g_pend_mode = mode; s->g_pend_k = k;
  s->g_pend = mode <= 1 ? 1u : (mode == 2 || mode == 3) ? 2u : mode == 5 ? 3u : (mode >= 6 && mode <= 9) ? 4u : 0u;      // (HRDT decides in its own launch)
  return 1;
}

// the step's likelihood: the engine's general kernels over the records the step kernel wrote
static int gb_eval(bpa_sampler * s, int kind)
{
  bpa_engine * e = s->eng;
  if (!e->usedata) return 1;
  PlanDev d{};
  d.loci = e->d_loci.p; d.bfbeta = e->bfbeta; d.task_locus = s->g_tlocus.p; d.task_pat_off = s->g_tpat.p; d.thr_task = s->b_thr.p;
  d.op_off = s->g_oprng.p; d.ops = s->g_ops20.p; d.root_clv = s->g_root20.p; d.root_scaler = s->g_rscaler.p;
  d.site_term = s->g_site.p; d.lnl = s->g_lnl.p; d.mat_task = s->g_mtask.p; d.mat_pmatrix = s->g_mpm.p; d.mat_length = s->g_len.p;
  d.nmat = s->nloci*s->g_maxmat; d.ntasks = s->nloci; d.npatterns = s->g_npat; d.pad = s->g_rmax;
  hipEvent_t k0 = nullptr, k1 = nullptr;
  if (s->timing_stride && (s->timing_phase++ % s->timing_stride) == 0)
  {
    if (s->timed.size() >= 4096 && !sampler_timing_drain(s)) return 0;
    bpa_sampler::Timed t{nullptr, nullptr, kind};
    HIPCHK(hipEventCreate(&t.e0)); HIPCHK(hipEventCreate(&t.e1));
    s->timed.push_back(t);
    k0 = t.e0; k1 = t.e1;
  }
  d.flags = 1u | 64u;
  hipLaunchKernelGGL(pmatrix_s4_kernel, dim3((d.nmat*s->g_rmax + BPA_BLOCK - 1)/BPA_BLOCK), dim3(BPA_BLOCK), 0, e->stream, d, (uint32_t)s->g_rmax);
  d.flags = 2u | 4u | 64u;
  hipExtLaunchKernelGGL(partials_lnl_s4_kernel, dim3((d.npatterns + BPA_BLOCK - 1)/BPA_BLOCK), dim3(BPA_BLOCK), 0, e->stream, k0, k1, 0, d);
  hipLaunchKernelGGL(lnl_reduce_wave_kernel, dim3(s->nloci), dim3(64), 0, e->stream, d);
  HIPCHK(hipGetLastError());
  s->launches += 3; s->g_evals++;
  return 1;
}

// the two leaves of the launch loop both samplers share (declared in sampler.hpp; gs_iterate, gs_dev_allloci, gs_mubar)
static inline int sampler_step(bpa_sampler * s, unsigned mode, unsigned k, double tau_u, double mix_c, double mix_lnc)
{
  return s->big ? gb_step(s, mode, k, tau_u, mix_c, mix_lnc) : gs_step(s, mode, k, tau_u, mix_c, mix_lnc);
}
static inline int sampler_eval(bpa_sampler * s, int kind) { return s->big ? gb_eval(s, kind) : gs_eval(s, kind); }

static int gb_initialize(bpa_sampler * s) { return gb_step(s, 5) && gb_eval(s, 1); }

static int gb_download(bpa_sampler * s)
{
  bpa_engine * e = s->eng;
  // (the settle launch of a pending substitution-parameter step is followed by big_par_kernel: the blocks and eigensystems
  //  are level with the settled values before a plan or bpa_batch_evaluate computes from them)
  if (!gb_step(s, 4) || !gs_prog_pull(s)) return 0;
  HIPCHK(hipMemcpyAsync(s->b_trees.data(), s->b_dev.p, s->nloci*sizeof(gbig::BTree), hipMemcpyDeviceToHost, e->stream));
  return gs_download_tail(s);
}
