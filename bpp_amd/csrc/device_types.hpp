// device_types.hpp — structures shared by the host engine and the gfx950 kernels.
//
// HBM layout.  Every locus owns contiguous slices of the engine's
// arenas; the kernels see them through one LocusDev record per locus:
//
//   inner CLV buffer c (clv index tips+c), 4-state  : clv[((c*R + k)*Np + n)*4 + s]
//       "pattern-major": for one (buffer, rate) the Np patterns are contiguous,
//       32 B per pattern, so lane n of a wave reads one aligned 32-B chunk and a
//       wave reads 2 KiB contiguous.
//   inner CLV buffer c, 20-state                    : clv[((c*R + k)*S + s)*Ld + n],  Ld = Np rounded up to 16
//       state-major planes so that lanes (patterns) are contiguous for each state; the plane stride is a whole
//       number of 128-byte lines, so every wave's 8-byte loads of a plane start on a line (with Ld = Np = 105 a
//       no-arithmetic kernel of this access shape streams 4.0 TB/s, with Ld = 112: 5.2 TB/s — tools/probe_bw.hip).
//   tip "CLVs" are never materialised: tip t keeps its state code per pattern
//       (uint8 for 4 states, uint32 for 20) and is expanded to 0.0/1.0 in registers
//       — arithmetic identical to the reference's one-hot tip CLVs (locus.c:525-559).
//   P-matrix p                                      : pmat[((p*R + k)*S + i)*S + j]   (reference layout);
//       JC69 loci keep only the pair (a, b) per (matrix, rate): pmat[(p*R + k)*2 + {0,1}]
//   weights | tips | parameters (| JC69 (a,b) table) of a locus are one contiguous block (1-3 cache lines)
//   scaler s                                        : scaler[s*Np + n]
//   parameters (doubles)                            : rates[R] | rate_weights[R] | param_idx[R] |
//                                                     per rate matrix m: freqs[S] | subst[S(S-1)/2] |
//                                                     eigenvals[S] | eigenvecs[S*S] | inv_eigenvecs[S*S]
#pragma once
#include <stdint.h>
#include <stdlib.h>

struct LocusDev
{
  double *   clv;        // inner CLV buffers
  double *   pmat;       // P-matrix buffers
  uint32_t * scaler;     // scale buffers (may be null)
  uint8_t *  tips;       // tip state codes: tips*Np entries of 1 B (S=4) or 4 B (S=20)
  uint32_t * weights;    // pattern weights [Np] (for diploid loci: unphased weights live in dip_*)
  double *   par;        // parameter block (see above)
  // diploid (locus.c:2586-2615); null when not diploid
  uint32_t * dip_count;  // resolutions per unphased pattern [unphased_length]
  uint32_t * dip_map;    // concatenated phased-pattern indices
  uint32_t * dip_weights;// weights of the unphased patterns
  uint32_t   np;         // patterns ("sites")
  uint32_t   tips_n;
  uint32_t   rate_cats;
  uint32_t   states;
  uint32_t   model;      // BPA_*_MODEL_*
  uint32_t   dtype;
  uint32_t   rate_matrices;
  uint32_t   unphased_length; // 0 when not diploid
  uint32_t   pstride;         // doubles per (P-matrix, rate): 16, or 2 for JC69 loci, whose matrices are
  uint32_t   ld;              // kept as their (diagonal a, off-diagonal b) pair (locus.c:2384-2411).  ld: CLV plane stride
                              // (patterns) of a 20-state locus; = np for 4-state loci (pattern-major, no planes)
};

// offsets inside the parameter block
__host__ __device__ inline uint32_t par_rates(uint32_t)            { return 0; }
__host__ __device__ inline uint32_t par_rate_weights(uint32_t R)   { return R; }
__host__ __device__ inline uint32_t par_param_idx(uint32_t R)      { return 2*R; }
__host__ __device__ inline uint32_t par_matrix_stride(uint32_t S)  { return S + S*(S-1)/2 + S + 2*S*S; }
__host__ __device__ inline uint32_t par_matrix(uint32_t R, uint32_t S, uint32_t m) { return 3*R + m*par_matrix_stride(S); }
__host__ __device__ inline uint32_t pm_freqs(uint32_t)             { return 0; }
__host__ __device__ inline uint32_t pm_subst(uint32_t S)           { return S; }
__host__ __device__ inline uint32_t pm_evals(uint32_t S)           { return S + S*(S-1)/2; }
__host__ __device__ inline uint32_t pm_evecs(uint32_t S)           { return pm_evals(S) + S; }
__host__ __device__ inline uint32_t pm_ievecs(uint32_t S)          { return pm_evecs(S) + S*S; }
__host__ __device__ inline uint32_t par_size(uint32_t R, uint32_t S, uint32_t M) { return 3*R + M*par_matrix_stride(S); }

// one node update; mirrors bpa_op_t (include/bpp_amd.h)
struct OpDev
{
  uint32_t parent_clv;
  int32_t  parent_scaler;
  uint32_t left_clv;
  uint32_t left_pmatrix;
  int32_t  left_scaler;
  uint32_t right_clv;
  uint32_t right_pmatrix;
  int32_t  right_scaler;
};

// Flattened descriptors of the fused single-launch path: everything a lane needs is
// one 16-byte-aligned record away (no pointer chasing through the locus table).
struct TaskRec            // 96-byte header followed by nops OpDev records
{
  double *   clv;
  double *   pmat;
  uint32_t * scaler;
  const uint8_t *  tips;
  const uint32_t * weights;
  const double *   par;
  uint32_t   np, tips_n, rate_cats, lane0;       // lane0: global lane of pattern 0
  uint32_t   nops, root_clv; int32_t root_scaler; uint32_t task;
  uint32_t   unphased_length, pat_off, locus, pstride;
};
struct MatRec             // one (branch, all rate categories) P-matrix update
{
  double *       dst;     // pmat + pmatrix_index*R*16
  const double * par;
  uint32_t       rate_cats, model, entry, pad;   // entry: index into mat_length[]
};

// ---- compact step records of the JC69 path (step_jc69_v2_kernel) ------------------------------------------------
// Everything that does not change from step to step lives in two ENGINE-level tables that every plan shares and
// that stay in L2 — one 16-byte entry per lane (pattern weight, the pattern's tip codes, position in the locus) and
// one 80-byte entry per locus ("slot": buffer addresses, sizes) — so a step only brings 16 B per locus + 16 B per
// node update + 8 B per fresh P-matrix from HBM, and the lane -> record hop is an index calculation.
struct LaneStatic { uint32_t slot, wgt, tipcodes, n_np_tips; };   // slot 0xffffffff: idle lane; n | np << 9 | tips << 18 | k << 23 | R << 26
                                                                  // (a locus takes np*R lanes: lane k*np + n = pattern n, rate category k)
struct SlotStatic
{
  double *   clv;
  double *   pmat;
  uint32_t * scaler;
  const double * par;
  uint32_t   np, tips_n, lane0, locus;       // lane0: global lane of pattern 0
  uint32_t   unphased_length, rate_cats, model, pstride;
  const uint8_t * tips;                      // tip state codes [tips][np]: read by loci of more than 8 tips (their codes do not fit the lane entry)
  double     rate0;                          // the locus's first category rate (the only one of a JC69 / one-category locus): the P-matrix
};                                           // lanes of step_jc69_v2_kernel read it here instead of chasing par
struct StepRec                               // 16 B, followed by the step's StepOps (16 B each)
{
  uint32_t task;                             // index of the locus in this plan, 0xffffffff: not part of it
  uint32_t pat_off;
  uint8_t  root_clv; int8_t root_scaler; uint8_t nops, pad0;
  uint32_t pad1;
};
struct StepOp                                // bpa_op_t with byte indices (<= 8 tips: 22 CLVs, 28 P-matrices)
{
  uint8_t parent_clv, left_clv, right_clv, left_pmatrix, right_pmatrix;
  int8_t  parent_scaler, left_scaler, right_scaler;
  int32_t left_e, right_e;                   // entry of mat_length[] when that child's P-matrix is updated in this step, else -1
};
struct MatRec2 { uint32_t slot, pmatrix; };  // a fresh P-matrix of the step: (a, b) pair pmatrix of that slot

// a resident batched step (bpa_plan_t) as the kernels see it
struct PlanDev
{
  const LocusDev * loci;        // engine locus table
  const uint32_t * task_locus;  // [T] locus id of task t
  const uint32_t * task_pat_off;// [T+1] prefix of pattern counts
  const uint32_t * thr_task;    // [P] task of pattern-thread g
  const uint32_t * mat_off;     // [T+1]
  const uint32_t * mat_task;    // [M] task of branch entry e
  const uint32_t * mat_pmatrix; // [M]
  const double *   mat_length;  // [M]
  const uint32_t * op_off;      // [T+1]
  const OpDev *    ops;         // [O]
  const uint32_t * root_clv;    // [T]
  const int32_t *  root_scaler; // [T]
  double *         site_term;   // [P] per-pattern weighted log-likelihood (or likelihood for diploid loci)
  double *         lnl;         // [T]
  // fused single-launch path (all loci of the plan fit a workgroup): workgroup b owns the
  // whole tasks blk_task_off[b]..blk_task_off[b+1); lane l of it owns pattern
  // (lane_task[b*BS+l], b*BS + l - task_lane0[task]) or nothing (0xffffffff)
  const uint32_t * blk_task_off;// [B+1]
  const uint32_t * lane_task;   // [B*BS]
  const uint32_t * task_lane0;  // [T] global lane index of the task's pattern 0
  const uint32_t * lane_rec;    // [B*BS] offset (16-byte units) of the lane's TaskRec in recs, or 0xffffffff
  const uint4 *    recs;        // TaskRec records
  const MatRec *   mat_recs;    // [M]
  const uint32_t * task_rec;    // [T] record offset of task t
  // tiled path (20 states): workgroup b owns patterns tile_n0[b] .. +TILE of task tile_task[b]
  const uint32_t * tile_task;   // [NT]
  const uint32_t * tile_n0;     // [NT]
  uint32_t *       tile_arrive; // [T] flags bit 9 (partials_lnl_wave20_kernel): tiles of task t that have written their terms, ever (a multiple of the task's tile count between launches): the last one adds the locus's terms up
  // compact JC69 path
  const LaneStatic * lane_tab;  // engine table [B2*256]
  const SlotStatic * slot_tab;  // engine table [slots]
  const uint32_t * blk_slot_off;// engine table [B2+1]
  const uint4 *    recs2;       // [slots*rec2_units] StepRec + StepOps
  const MatRec2 *  mat2;        // [M]
  const uint32_t * blk_mat_off; // [B2+1] fresh P-matrices of the workgroup's loci
  uint32_t         rec2_units;  // 16-byte units per slot record
  uint32_t         nblocks2;
  double *         wg_part;     // [B2] flags bit 3: workgroup b's sum of its loci's lnL (bpa_plan_enable_partial_sums)
  unsigned long long * dbg;     // optional per-workgroup timestamps (profiling aid, normally null)
  uint32_t         nblocks;     // B (0: fused path not available)
  uint32_t         flags;       // bit0: compute P-matrices, bit1: node updates + site terms, bit2: per-locus lnL, bit3 (v2 kernel): + per-workgroup sums of them
  uint32_t         ntasks;
  uint32_t         npatterns;
  uint32_t         nmat;
  uint32_t         pad;
  uint32_t         blk0;        // compact path: the launch covers workgroups blk0 .. blk0 + gridDim.x of the packing (a half-batch launch)
  uint32_t         ent0;        // dense P-matrix launch: first branch entry of the launch's range
  double           bfbeta;
};
