// Initialisation and reset of the batch: references, per-problem solver state and the PD warm
// start (k_init), the AL / ReB and option values of handles with more than one set
// (k_init_params), memory_reset for the batch (k_reset_arrays) and for a list of problems
// (k_scatter_x0, k_reset_list: mhpc_reset_problems).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mhpc_device.h"
#include "mhpc_launch.h"
#include "mhpc_model_pair.h"

namespace MHPC_NS {

// ============================================================================================
// initialization: references, state, PD warm start (MHPCLocomotion.cpp:47-53,200-215)
// ============================================================================================
// warm = 0 (mhpc_update_problem): references and per-problem state only -- the reference's
// update_problem() regenerates the references and re-initialises the AL / ReB parameters of
// every phase but keeps the (rotated) nominal trajectories and gains as the warm start.
// References (ReferenceGen.h:94-109) and the per-problem solver state of one problem;
// warm = 1 also resets the option fields a solve rewrites (see ProbState).
// AL_REB_PARAMETER of phase p's mode (MHPCConstraints.cpp:43-88, mhpc_set_constraint_params)
static __device__ __forceinline__ void init_al_reb(ProbState* st, const Layout& L,
                                                   const CostParams& cw, int p) {
  const bool wb = p < L.n_wb && p < L.P;
  const int m = p < L.P ? L.mode[p] - 1 : 0;
  st->sigma[p] = (wb && ntc_of(L.mode[p], true)) ? cw.sigma0[m] : real(0.0);
  st->delta[p] = cw.delta0[m];
  st->eps_tq[p] = cw.eps_tq0[m];
  st->eps_grf[p] = cw.eps_grf0[m];
}
__device__ void k_init_state(const SolveParams& sp, const DevBufs& d, const Layout& L, int b,
                             int warm) {
  const real* x0 = d.x0 + (size_t)b * 14;
  real* pos = d.refpos + (size_t)b * sp.NK;
  const real vel = cmd_of(d, b).vel;
  for (int p = 0; p < L.P; ++p) {
    const int ko = L.ko[p];
    pos[ko] = p == 0 ? x0[0] : pos[L.ko[p - 1] + L.N[p - 1] - 1];
    for (int k = 1; k < L.N[p]; ++k) pos[ko + k] = pos[ko + k - 1] + vel * L.dt[p];
  }
  ProbState* st = &d.st[b];
  st->J = 0; st->viol = 0; st->dV_exp = 0; st->reg = 0; st->cost_prev = 0;
  for (int p = 0; p < MAXP; ++p) {
    st->V[p] = 0; st->dV[p] = 0; st->h[p] = 0; st->lambda[p] = 0;
    init_al_reb(st, L, sp.cw, p);  // (problem 0's set: see k_init_params)
  }
  st->status = MHPC_SOLVE_OK;
  // ReB flag as the options set it (what a sweep right after initialization() sees); the
  // first forward_sweep(0) applies the per-AL-iteration rule (MultiPhaseDDP.cpp:178-183)
  st->active = 1; st->ddp_active = 0; st->reb_active = sp.ReB_active ? 1 : 0; st->al_partials = 0;
  st->nom_slot = 0; st->al_iter = 0; st->ddp_iter = 0; st->bws_iter = 0; st->ntrace = 0;
  for (int i = 0; i < TRACE; ++i) st->trace[i] = -1;
  for (int i = 0; i < NCNT; ++i) st->cnt[i] = 0;
  st->par_slot = 0;
  st->par_al = 0;
  st->ls_nt = 0;
  st->ls_nom = 0;
  st->reroll_j = -1;
  st->reroll_nom = 0;
  st->reroll_eps = real(0.0);
  for (int p = 0; p < MAXP; ++p) {
    st->par_sigma[p] = 0; st->par_lambda[p] = 0; st->ls_sigma[p] = 0; st->ls_lambda[p] = 0;
  }
  if (!warm) return;
  st->opt_reb = sp.ReB_active ? 1 : 0;
  st->opt_pen = sp.update_penalty;
  st->cap_reb = st->opt_reb;
  st->cap_pen = st->opt_pen;
}

// A lane pair per problem (even lane: front leg, odd: back leg of the pair dynamics,
// mhpc_model_pair.h): the warm-start rollout is one serial chain per problem, so halving its
// per-knot latency is what counts; both lanes carry the same state and controls (the pair
// model returns xdot and y on both, bit for bit the single-lane model's), the even lane
// writes the references and the per-problem state, each lane half of every knot record.
// memory_reset (MHPCLocomotion.cpp:265-288), launched on the second stream beside k_init and
// hidden behind its serial warm-start chains: K, du and G of every knot, and u and y of
// every phase's last knot in every trajectory slot (no rollout writes them, quirk B11; a slot
// becoming the nominal carries them into the exports).  Everything else of traj is written
// before it is read (slot 0 by k_init, the candidate slots by the line search), so initialize
// does not clear the whole array (2.8 GB at batch 4096).  k_init reads none of these arrays
// and writes other elements of the tail records.
__device__ void init_reset_arrays(const SolveParams& sp, const DevBufs& d, long t, long nt) {
  const long nk = (long)sp.B * sp.NK;
  for (long i = t; i < nk * 56; i += nt) d.K[i] = real(0.0);
  for (long i = t; i < nk * 4; i += nt) d.du[i] = real(0.0);
  for (long i = t; i < nk * 14; i += nt) d.G[i] = real(0.0);
  const long n = (long)sp.B * sp.nslot * sp.pmax;
  for (long i = t; i < n; i += nt) {
    const int p = (int)(i % sp.pmax);
    const long bs = i / sp.pmax;
    const int slot = (int)(bs % sp.nslot), b = (int)(bs / sp.nslot);
    const Layout& L = d.grp[d.lid[b]].lay;  // the problem's layout (per lane; hidden beside k_init)
    if (p >= L.P) continue;
    const int nx = p < L.n_wb ? 14 : 6;
    real* r = traj_ptr(sp, d, b, slot, L.ko[p] + L.N[p] - 1);
    for (int e = nx; e < KS; ++e) r[e] = real(0.0);
  }
}

__global__ __launch_bounds__(256) void k_reset_arrays(SolveParams sp, DevBufs d) {
  init_reset_arrays(sp, d, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}

// ---- per-problem re-initialisation (mhpc_reset_problems): list-driven, work ~ n not B ----------
// The padded x0 rows [n][14] of the listed problems to their device rows.
__global__ __launch_bounds__(64) void k_scatter_x0(DevBufs d, int n, const int* list,
                                                   const real* rows) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n * 14) return;
  d.x0[(size_t)list[t / 14] * 14 + t % 14] = rows[t];
}

// memory_reset of the listed problems: what k_reset_arrays does for the batch (K, du, G over the
// whole knot stride; u, y of every phase's last knot in every slot, by the problem's current
// layout) and, when the phase-buffer store exists, their store rows (ensure_store's memset for
// one problem).  A block per (listed problem, chunk of RL_CH items): item t is knot t of the
// stride and record t of the problem's spmax * nbk store records (spmax = 0 without a store;
// nch = chunks per problem over the longer of the two).  A chunk's K, du, G and store records are
// contiguous, so the block's lanes stride over their elements (whole lines per wave).
constexpr int SREC = kStoreRec;  // reals of a store record (mhpc_store.hip)
constexpr int RL_CH = 64;
__global__ __launch_bounds__(256) void k_reset_list(SolveParams sp, DevBufs d, const int* list,
                                                    int nch, real* store, int nbk, int spmax) {
  const int b = list[blockIdx.x / nch], i0 = (int)(blockIdx.x % nch) * RL_CH, t = threadIdx.x;
  const int k1 = min(i0 + RL_CH, sp.NK);
  if (i0 < k1) {
    const size_t r0 = (size_t)b * sp.NK + i0;
    const int nk = k1 - i0;
    for (int e = t; e < nk * 56; e += 256) d.K[r0 * 56 + e] = real(0.0);
    for (int e = t; e < nk * 4; e += 256) d.du[r0 * 4 + e] = real(0.0);
    for (int e = t; e < nk * 14; e += 256) d.G[r0 * 14 + e] = real(0.0);
    const Layout& L = d.grp[d.lid[b]].lay;
    for (int e = t; e < L.P * sp.nslot; e += 256) {  // a lane per (phase, slot) tail
      const int p = e / sp.nslot, slot = e % sp.nslot;
      const int kk = L.ko[p] + L.N[p] - 1;
      if (kk < i0 || kk >= k1) continue;
      real* r = traj_ptr(sp, d, b, slot, kk);
      for (int q = p < L.n_wb ? 14 : 6; q < KS; ++q) r[q] = real(0.0);
    }
  }
  const int s1 = min(i0 + RL_CH, spmax * nbk);
  if (i0 < s1) {
    real* o = store + ((size_t)b * spmax * nbk + i0) * SREC;
    for (int e = t; e < (s1 - i0) * SREC; e += 256) o[e] = real(0.0);
  }
}

// The AL / ReB initial values of every problem from its group's parameter record, after k_init
// (which wrote problem 0's set for all): launched only when the handle holds more than one set
// (mhpc_set_param_sets).  k_init keeps its own read of the parameter block, SolveParams::cw:
// with that read gone or moved to the table the fp32 build's SLP vectoriser packs the
// warm-start rollout below differently, three of its multiply-adds no longer contract, and
// every fp32 result changes in the last bits (k_init has no MHPC_NO_FMA_F32: its rounding is
// part of the fp32 results as they stand).
// The same holds for the option fields k_init_state writes (the ReB flag; warm: the fields a
// solve rewrites): k_init writes problem 0's record for all, from SolveParams::ReB_active /
// update_penalty, and with more than one option set (mhpc_set_option_sets) this kernel then
// writes each problem's own.  warm: as k_init's.
// A problem whose record has no AL iteration (n_al = 0) never runs forward_sweep(0): in the
// reference its SRB phases keep the zero states memory_reset left, since only that first sweep
// rolls them out.  k_init completed them ahead of that sweep (see there), so with warm the states
// of its SRB knots in slot 0 go back to zero here (their u and y are zero already); the host
// makes the problem's first forward_sweep(0) the real rollout should its budget be raised before
// its next solve (Handle::srb_open).
__global__ __launch_bounds__(64) void k_init_params(SolveParams sp, DevBufs d, int warm) {
  const GrpBlk gb = block_group(sp, blockIdx.x, 64);
  if (gb.g < 0 || gb.p0 + (int)threadIdx.x >= gb.p1) return;
  const Layout& L = layout_of(d, gb.g);
  const CostParams& cw = params_of(d, gb.g);
  const int b = prob_at(sp, d, gb.p0 + threadIdx.x);
  ProbState* st = &d.st[b];
  for (int p = 0; p < MAXP; ++p) init_al_reb(st, L, cw, p);
  const OptRec& o = opt_of(d, b);
  st->reb_active = o.ReB_active ? 1 : 0;
  if (!warm) return;
  st->opt_reb = o.ReB_active ? 1 : 0;
  st->opt_pen = o.update_penalty;
  st->cap_reb = st->opt_reb;
  st->cap_pen = st->opt_pen;
  if (o.n_al == 0)
    for (int p = L.n_wb; p < L.P; ++p)
      for (int k = 0; k < L.N[p]; ++k) {
        real* r = traj_ptr(sp, d, b, 0, L.ko[p] + k);
        for (int i = 0; i < 6; ++i) r[i] = real(0.0);
      }
}

__global__ __launch_bounds__(64) void k_init(SolveParams sp, DevBufs d, int warm) {
  // blocks by group, 32 problems a block
  const GrpBlk gb = block_group(sp, blockIdx.x, 32);
  const int i0 = threadIdx.x >> 1;
  const bool back = (threadIdx.x & 1) != 0;
  if (gb.g < 0 || gb.p0 + i0 >= gb.p1) return;  // both lanes of a pair
  const Layout& L = layout_of(d, gb.g);
  const int b = prob_at(sp, d, gb.p0 + i0);
  const real* x0 = d.x0 + (size_t)b * 14;
  if (!back) k_init_state(sp, d, L, b, warm);
  if (!warm) return;
  // warm start of the WB phases into slot 0 (bounding_PDcontrol, boundingPDControl.cpp:3-46)
  real x[14];
  for (int i = 0; i < 14; ++i) x[i] = x0[i];
  const real qnom[4] = {PI / 4, -PI * 7 / 12, PI / 4, -PI * 7 / 12};
  const real Kp[4] = {5 * real(8.0), 5 * real(1.0), 5 * real(12.0), 5 * real(10.0)};
  SinCosK scK = kSinCosK;  // VGPR copies (see k_rollout)
  MHPC_PIN_VGPRS(scK);
  for (int p = 0; p < L.n_wb; ++p) {
    const int mode = L.mode[p], N = L.N[p], ko = L.ko[p];
    const real dt = L.dt[p];
    for (int k = 0; k < N - 1; ++k) {
      // the state-only part of the dynamics first: the stance controller reuses its geometry
      WbPairPrep P;
      wb_pair_prep(x, back, P, scK);
      real u[4];
#ifdef MHPC_FP32
      // (fp32: the reference-ordered evaluation below; its C5 accuracy is chaotic in the warm
      // start's last bits -- the pair-geometry form moved the X 95th percentile of
      // tests/test_gpu_fp32.py from 7.9e-3 to 1.2e-2, past the 1e-2 target)
      if (mode == 1 || mode == 3) {
        real J[14], Jd[14], v[2];
        if (mode == 1) { wb_foot_jacobian_f<kBack>(x, J, Jd); wb_leg_ext<kBack>(x, v); }
        else { wb_foot_jacobian_f<kFront>(x, J, Jd); wb_leg_ext<kFront>(x, v); }
        const real sq = v[0] * v[0] + v[1] * v[1], nrm = sqrt(sq);
        const real n0 = v[0] / nrm, n1 = v[1] / nrm;
        const real F0 = -n0 * real(2200.0) * (nrm - real(0.2462)), F1 = -n1 * real(2200.0) * (nrm - real(0.2462));
        const real gain = mode == 1 ? 3 : real(2.2);
        for (int i = 0; i < 4; ++i) u[i] = (J[3 + i] * F0 + J[7 + 3 + i] * F1) * gain;
      }
#else
      if (mode == 1 || mode == 3) {
        // the stance foot's Jacobian (wb_foot_jacobian_f: its leg's hip / knee columns; the
        // other leg's are exact zeros) and hip-to-foot vector (wb_leg_ext) from the stance
        // lane's own-leg geometry -- the same expressions on the same sines / cosines
        const bool mine = (mode == 1) == back;
        real jx[5], jz[5], jdx, jdz;
        pair_point_jac(P.L, P.sg, P.sth, P.cth, kThighLen, kShankLen, jx, jz, &jdx, &jdz);
        const real ve0 = -kThighLen * P.L.s1 - kShankLen * P.L.s2;
        const real ve1 = -kThighLen * P.L.c1 - kShankLen * P.L.c2;
        const real v[2] = {mode == 1 ? pair_from<1>(ve0) : pair_from<0>(ve0),
                           mode == 1 ? pair_from<1>(ve1) : pair_from<0>(ve1)};
        const real sq = v[0] * v[0] + v[1] * v[1], nrm = sqrt(sq);
        const real n0 = v[0] / nrm, n1 = v[1] / nrm;
        const real F0 = -n0 * real(2200.0) * (nrm - real(0.2462)), F1 = -n1 * real(2200.0) * (nrm - real(0.2462));
        const real gain = mode == 1 ? 3 : real(2.2);
        real uo[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const real jxa = mine ? jx[3 + a] : real(0.0), jza = mine ? jz[3 + a] : real(0.0);
          uo[a] = (jxa * F0 + jza * F1) * gain;
        }
        u[0] = pair_from<0>(uo[0]); u[1] = pair_from<0>(uo[1]);
        u[2] = pair_from<1>(uo[0]); u[3] = pair_from<1>(uo[1]);
      }
#endif
      else {
        for (int i = 0; i < 4; ++i) u[i] = Kp[i] * (qnom[i] - x[3 + i]) - x[10 + i];
      }
      const real u2[2] = {back ? u[2] : u[0], back ? u[3] : u[1]};
      real xd[14], y[4];
      wb_pair_finish(x, u2, mode, back, P, xd, y);
      // record x (14) u (4) y (4): even lane entries 0..10, odd lane 11..21
      real rec[22];
      for (int i = 0; i < 14; ++i) rec[i] = x[i];
      for (int i = 0; i < 4; ++i) { rec[14 + i] = u[i]; rec[18 + i] = y[i]; }
      real* o = traj_ptr(sp, d, b, 0, ko + k) + (back ? 11 : 0);
#pragma unroll
      for (int i = 0; i < 11; ++i) o[i] = back ? rec[11 + i] : rec[i];
      for (int i = 0; i < 14; ++i) x[i] = x[i] + xd[i] * dt;
    }
    real* oe = traj_ptr(sp, d, b, 0, ko + N - 1);
    if (!back) for (int i = 0; i < 14; ++i) oe[i] = x[i];
    wb_phase_transition(L, p, x);  // the forward sweep's
  }
  // SRB phases: the reference's first forward_sweep(0) rolls them out with the initial
  // (zero) controls and zero gains -- u = (0 + 0*0) + sum 0*(x - 0) = +0 exactly -- so the
  // nominal is completed here and forward_sweep(0) reduces to a cost evaluation (k_cost).
  // Both lanes run the (cheap) SRB chain; each writes half of every record.
  if (L.n_wb == 0)
    for (int i = 0; i < 6; ++i) x[i] = x0[i];
  for (int p = L.n_wb; p < L.P; ++p) {
    const int mode = L.mode[p], N = L.N[p], ko = L.ko[p];
    const real dt = L.dt[p];
    real f[4], s[2];
    plan_foothold(x, dt * N, mode, f);
    srb_contact(mode, s);
    const real u[4] = {real(0.0), real(0.0), real(0.0), real(0.0)};
    for (int k = 0; k < N - 1; ++k) {
      real xd[6];
      srb_dynamics(x, u, f, s, xd);
      real rec[14];
      for (int i = 0; i < 6; ++i) rec[i] = x[i];
      for (int i = 0; i < 4; ++i) { rec[6 + i] = u[i]; rec[10 + i] = real(0.0); }
      real* o = traj_ptr(sp, d, b, 0, ko + k) + (back ? 7 : 0);
#pragma unroll
      for (int i = 0; i < 7; ++i) o[i] = back ? rec[7 + i] : rec[i];
      for (int i = 0; i < 6; ++i) x[i] = x[i] + xd[i] * dt;
    }
    real* oe = traj_ptr(sp, d, b, 0, ko + N - 1);
    if (!back) for (int i = 0; i < 6; ++i) oe[i] = x[i];
  }
}

// ---- launchers (called by mhpc_runtime.cpp) ---------------------------------------------
hipError_t launch_reset(const SolveParams& sp, const DevBufs& d, hipStream_t s) {
  hipLaunchKernelGGL(k_init, dim3(grid_of(sp, 32)), dim3(64), 0, s, sp, d, 0);
  return hipGetLastError();
}
hipError_t launch_reset_arrays(const SolveParams& sp, const DevBufs& d, hipStream_t s) {
  // ~64 elements per lane, at most 2 blocks per CU
  const long e = (long)sp.B * sp.NK * 74 + (long)sp.B * sp.nslot * sp.pmax;
  const long nb = std::min((e + 256 * 64 - 1) / (256 * 64), 2L * sp.ncu);
  hipLaunchKernelGGL(k_reset_arrays, dim3((unsigned)nb), dim3(256), 0, s, sp, d);
  return hipGetLastError();
}
hipError_t launch_scatter_x0(const DevBufs& d, int n, const int* list, const real* rows,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_scatter_x0, dim3((unsigned)((n * 14L + 63) / 64)), dim3(64), 0, s, d, n, list,
                     rows);
  return hipGetLastError();
}
// store == nullptr: no phase-buffer store yet (nbk, spmax ignored)
hipError_t launch_reset_list(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                             real* store, int nbk, int spmax, hipStream_t s) {
  if (!store) nbk = spmax = 0;
  const int nch = (std::max(sp.NK, spmax * nbk) + RL_CH - 1) / RL_CH;
  hipLaunchKernelGGL(k_reset_list, dim3((unsigned)n * nch), dim3(256), 0, s, sp, d, list, nch, store,
                     nbk, spmax);
  return hipGetLastError();
}
hipError_t launch_init_params(const SolveParams& sp, const DevBufs& d, int warm, hipStream_t s) {
  hipLaunchKernelGGL(k_init_params, dim3(grid_of(sp, 64)), dim3(64), 0, s, sp, d, warm);
  return hipGetLastError();
}
hipError_t launch_init(const SolveParams& sp, const DevBufs& d, hipStream_t s) {
  hipLaunchKernelGGL(k_init, dim3(grid_of(sp, 32)), dim3(64), 0, s, sp, d, 1);
  return hipGetLastError();
}

}  // namespace MHPC_NS
