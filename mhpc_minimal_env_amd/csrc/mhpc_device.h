// Device-side helpers shared by the solve kernels: cost weights, references, reduced
// barrier, running and terminal costs, phase transition, foothold planner.  Every helper
// restates reference code cited at its definition.
#pragma once
#include <hip/hip_runtime.h>

#include "mhpc_model.h"
#include "mhpc_solver.h"

namespace MHPC_NS {

constexpr real PI = real(3.141592653589793238);  // MHPC_CPPTypes.h:18

// Cost weights and constraint parameters are the block's group record (params_of below;
// mhpc_set_cost_weights / mhpc_set_constraint_params / mhpc_set_param_sets; defaults
// MHPCCost.cpp:24-75, MHPCConstraints.cpp:14-88).
// terminal WB state references (ReferenceGen.cpp:45-52), velocity entry filled at run time
static __constant__ real cXtermWB[4][14] = {
    {0, -real(0.1432), -PI / 25, real(0.35) * PI, -real(0.65) * PI, real(0.35) * PI, -real(0.6) * PI, 0, 1, 0, 0, 0, 0, 0},
    {0, -real(0.1418), PI / 35, real(0.2) * PI, -real(0.58) * PI, real(0.25) * PI, -real(0.7) * PI, 0, -1, 0, 0, 0, 0, 0},
    {0, -real(0.1325), -PI / 40, real(0.33) * PI, -real(0.48) * PI, real(0.33) * PI, -real(0.75) * PI, 0, 1, 0, 0, 0, 0, 0},
    {0, -real(0.1490), -PI / 25, real(0.35) * PI, -real(0.7) * PI, real(0.25) * PI, -real(0.60) * PI, 0, -1, 0, 0, 0, 0, 0}};
static __constant__ real cQjointBias[4] = {real(0.3) * PI, -real(0.7) * PI, real(0.3) * PI, -real(0.7) * PI};
constexpr real kGRF = real(8.252) * real(9.81);  // ReferenceGen.cpp:27

static __device__ __forceinline__ real* traj_ptr(const SolveParams& sp, const DevBufs& d, int b,
                                            int slot, int kk) {
  return d.traj + (((size_t)b * sp.nslot + slot) * sp.NK + kk) * KS;
}

static __device__ __forceinline__ int ntc_of(int mode, bool wb) { return wb && (mode == 2 || mode == 4); }

// Feedback term K[i] (x - x_nom) of the line-search control (SinglePhase.cpp forward sweep,
// u = u_nom + eps du + K dx), summed in column order.  (Summing the two halves of the row
// separately -- a chain half as long -- measured no faster: profiles/r02_ab_wt_layout.txt.)
// Shared by the rollouts (mhpc_kernels.hip) and the one-knot control law of mhpc_control
// (mhpc_control.hip), whose u must equal a rollout's bit for bit.
template <int N>
__device__ __forceinline__ real fb_dot(const real* Kr, const real* x, const real* nk) {
  MHPC_NO_FMA_F32  // as in the kernels that call it (fp32 line search uncontracted)
  real fb = 0;
#pragma unroll
  for (int c = 0; c < N; ++c) fb += Kr[c] * (x[c] - nk[c]);
  return fb;
}

// ---- groups: (layout, parameter set) pairs ------------------------------------------------
// A launch over the batch enumerates its blocks group by group: group g (problems
// gidx[go[g] .. go[g+1]), record grp[g]) takes ceil(n_g / per) blocks of `per` problems, so every
// wave of a block runs one layout (uniform control flow, the layout in scalar registers).
struct GrpBlk {
  int g;       // group (-1: block past the last group)
  int p0, p1;  // the block's first gidx position and the end of its group's positions
};
static __device__ __forceinline__ GrpBlk block_group(const SolveParams& sp, int blk, int per) {
  int start = 0;
  for (int g = 0; g < sp.ngrp; ++g) {
    const int n = sp.go[g + 1] - sp.go[g], nb = (n + per - 1) / per;
    if (blk < start + nb) return {g, sp.go[g] + (blk - start) * per, sp.go[g + 1]};
    start += nb;
  }
  return {-1, 0, 0};
}
// The same for launches of `per_item` items per problem (e.g. the partials' knots) in blocks
// of `nt` lanes: group g takes ceil(n_g * items_g / nt) blocks; *t0 = the block's first item
// of the group (problem position go[g] + item / items_g).
// (items == nullptr: n_items for every group)
static __device__ __forceinline__ int block_group_items(const SolveParams& sp, const int* items,
                                                         int n_items, int blk, int nt, long* t0) {
  int start = 0;
  for (int g = 0; g < sp.ngrp; ++g) {
    const long n = (long)(sp.go[g + 1] - sp.go[g]) * (items ? items[g] : n_items);
    const int nb = (int)((n + nt - 1) / nt);
    if (blk < start + nb) {
      *t0 = (long)(blk - start) * nt;
      return g;
    }
    start += nb;
  }
  return -1;
}
// Problem index at gidx position pos.
static __device__ __forceinline__ int prob_at(const SolveParams& sp, const DevBufs& d, int pos) {
  return sp.ident ? pos : d.gidx[pos];
}
// The lane's (group, problem, item) in a launch of n items per problem, 64 lanes a block, blocks
// by group (block_group_items), the item index fastest; false: the lane has none.
static __device__ __forceinline__ bool lane_item(const SolveParams& sp, const DevBufs& d, int n,
                                                 int* g, int* b, int* e) {
  long t0 = 0;
  *g = block_group_items(sp, nullptr, n, blockIdx.x, 64, &t0);
  if (*g < 0) return false;
  const long tg = t0 + threadIdx.x;  // item within the group
  if (tg >= (long)(sp.go[*g + 1] - sp.go[*g]) * n) return false;
  *b = prob_at(sp, d, sp.go[*g] + (int)(tg / n));
  *e = (int)(tg % n);
  return true;
}
// Record of group g, read through the constant address space: the table never changes during a
// launch, so every field a wave-uniform index selects is a scalar load (s_load), as a
// parameter-block field would be, never a vector load plus readfirstlane.  layout_of / params_of
// are its two halves, addressed from the one base; read them only once the block knows it has
// a group.
typedef const __attribute__((address_space(4))) Group CGroup;
static __device__ __forceinline__ const Layout& layout_of(const DevBufs& d, int g) {
  return *(const Layout*)&((CGroup*)d.grp + g)->lay;
}
// Cost weights and constraint parameters of group g (its parameter set).
static __device__ __forceinline__ const CostParams& params_of(const DevBufs& d, int g) {
  return *(const CostParams*)&((CGroup*)d.grp + g)->cw;
}

// User command of problem b: loaded once per problem where a kernel picks up its state (the
// cost code and the sweep fold it into their per-lane references, never a load per knot).
static __device__ __forceinline__ Cmd cmd_of(const DevBufs& d, int b) { return d.cmd[b]; }

// Option record of problem b: read where the per-problem control flow needs a field (per lane:
// the problems of a wave may differ), never inside a knot loop.  The only index that depends on
// it is this table lookup (oid[b] < MAXO by the host's construction).
static __device__ __forceinline__ const OptRec& opt_of(const DevBufs& d, int b) {
  return d.opt[d.oid[b]];
}
// Problem b takes part in op (al, ddp) of a solve schedule: the schedule of a scope runs to the
// largest caps among its problems, and a problem with smaller ones sits the rest out exactly as in
// a handle of its own, where those ops are never issued.
static __device__ __forceinline__ bool in_op(const OptRec& o, int al, int ddp) {
  return al <= o.n_al && ddp <= o.max_ddp;
}
// The same for problem b of a launch of the solve schedule: an op within the scope's smallest caps
// (uniform, from the parameter block) takes everybody and reads nothing.
static __device__ __forceinline__ bool in_op(const SolveParams& sp, const DevBufs& d, int b, int al,
                                             int ddp) {
  if (al <= sp.min_n_al && ddp <= sp.min_max_ddp) return true;
  return in_op(opt_of(d, b), al, ddp);
}
// AL_active of problem b in such a launch: the scope's common value, or the record's.
static __device__ __forceinline__ bool al_active_of(const SolveParams& sp, const DevBufs& d, int b) {
  return sp.al_uniform >= 0 ? sp.al_uniform != 0 : opt_of(d, b).AL_active != 0;
}

// Natural log of a positive argument (the barrier's g > delta > 0 and delta itself).  fp64:
// the fdlibm algorithm (e_log.c: x = 2^k (1 + f) with sqrt(2)/2 <= 1 + f < sqrt(2),
// s = f / (2 + f), a degree-14 odd polynomial in s), < 1 ulp on every positive finite argument,
// subnormals included (frexp scales them), and log_pos(1) = +0 (tests/test_gpu_primitives.py
// against a 60-digit reference) -- about a third of the instructions of the library log, whose
// extra work covers special values this path never sees.  log_pos(+inf) is NaN (f / (2 + f) is
// inf / inf) where the library gives +inf: a barrier argument of +inf, which no constraint of
// the model is known to reach, gives B = NaN where the reference has -inf (the test records
// it as an expected failure; a select on the result cost 0.5 % of the C3 solve).  The line
// search evaluates up to 11 of these per WB knot and candidate while the ReB barrier is
// active.
static __device__ __forceinline__ real log_pos(real x) {
  MHPC_NO_FMA_F32
#ifdef MHPC_FP32
  return logf(x);
#else
  int k;
  double m = frexp(x, &k);  // x = m 2^k, m in [0.5, 1)
  const bool lo = m < 0.70710678118654752440;
  m = lo ? m + m : m;
  k = lo ? k - 1 : k;
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 +
                                                         w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 +
                         w * (2.857142874366239149e-01 +
                              w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  const double dk = (double)k;
  return dk * 6.93147180369123816490e-01 -
         ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
#endif
}

// ---- reduced barrier (SinglePhase.cpp:298-317), k = 2 ---------------------------------
// The reference's pow() calls with integer exponents are evaluated exactly as products:
// pow(t, 2) = t*t (the correctly rounded square), pow(t, 1) = t, pow(t, 0) = 1 (also for
// NaN, as pow defines), pow(g, -2) = 1/(g*g) (within 1 ulp of the correctly rounded value).
// One log per constraint (of g or of delta, whichever side the lane takes) outside the branch,
// so a wave whose lanes split over the two sides evaluates one log, not both; the relaxed
// side's extra work stays behind a branch that waves far from the constraint skip.  Each lane
// computes exactly the operations of its side.
static __device__ __forceinline__ void reduced_barrier(real g, real delta, real* B, real* Bz,
                                                real* Bzz) {
  MHPC_NO_FMA_F32
  const bool in = g > delta;
  const real lg = log_pos(in ? g : delta);
  if (in) {
    *B = -lg;
    *Bz = -1.0 / g;
    *Bzz = 1.0 / (g * g);
  } else {
    const real t = (g - 2 * delta) / ((2 - 1) * delta);
    *B = (real)(2 - 1) / 2 * (t * t - 1) - lg;
    *Bz = t / delta;
    *Bzz = 1.0;
  }
}

// Running state reference of a WB / SRB knot (ReferenceGen.h:53-92: forward position, commanded
// height and speed, nominal joint angles), built in registers.
static __device__ __forceinline__ void wb_run_ref(const Cmd& cm, real pos, real* rx) {
  MHPC_NO_FMA_COST
  rx[0] = pos; rx[1] = cm.height; rx[2] = 0;
  rx[3] = cQjointBias[0]; rx[4] = cQjointBias[1]; rx[5] = cQjointBias[2]; rx[6] = cQjointBias[3];
  rx[7] = cm.vel;
#pragma unroll
  for (int i = 8; i < 14; ++i) rx[i] = 0;
}
static __device__ __forceinline__ void fb_run_ref(const Cmd& cm, real pos, real* rx) {
  MHPC_NO_FMA_COST
  rx[0] = pos; rx[1] = cm.height; rx[2] = 0; rx[3] = cm.vel; rx[4] = 0; rx[5] = 0;
}

// Running cost value incl. the ReB barrier of WB phases (CostBase.cpp:4-16,
// SinglePhase.cpp:219-249 in CALC_DYNAMICS_ONLY), reference of knot kk built in registers.
static __device__ __forceinline__ real wb_running_cost(const CostParams& cw, const Cmd& cm, int mode, real dt,
                                  real pos, const real* x, const real* u, const real* y, bool reb,
                                  real delta, real eps_tq, real eps_grf) {
  MHPC_NO_FMA_COST
  const int m = mode - 1;
  real rx[14];
  wb_run_ref(cm, pos, rx);
  const real ry[4] = {0, kGRF, 0, kGRF};
  real l = 0, t = 0;
#pragma unroll
  for (int i = 0; i < 14; ++i) { const real e = x[i] - rx[i]; l += e * cw.wQ[m][i] * e; }
#pragma unroll
  for (int i = 0; i < 4; ++i) { const real e = u[i]; t += e * cw.wR[m][i] * e; }
  l += t;
  t = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const real e = y[i] - ry[i]; t += e * cw.wS[m][i] * e; }
  l += t;
  l = l * dt;
  if (reb) {
    real B, Bz, Bzz;
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // torque limits tq_lim -/+ u
      const real g = (i < 4 ? -u[i] : u[i - 4]) + cw.tq_lim;
      reduced_barrier(g, delta, &B, &Bz, &Bzz);
      l += eps_tq * B * dt;
    }
    // joint limits carry eps_ReB = 0 (MHPCConstraints.cpp:64-84): contribution 0 * B * dt
    if (mode == 1 || mode == 3) {  // GRF: Fz >= 0, mu Fz -/+ Fx >= 0
      const int o = mode == 1 ? 2 : 0;
      const real mu = cw.mu;
      const real gs[3] = {y[o + 1], -y[o] + mu * y[o + 1], y[o] + mu * y[o + 1]};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        reduced_barrier(gs[i], delta, &B, &Bz, &Bzz);
        l += eps_grf * B * dt;
      }
    }
  }
  return l;
}

static __device__ __forceinline__ real fb_running_cost(const CostParams& cw, const Cmd& cm, int mode, real dt,
                                  real pos, const real* x, const real* u) {
  MHPC_NO_FMA_COST
  const int m = mode - 1;
  real rx[6];
  fb_run_ref(cm, pos, rx);
  const real ru[4] = {0, kGRF, 0, kGRF};
  real l = 0, t = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) { const real e = x[i] - rx[i]; l += e * cw.fQ[m][i] * e; }
#pragma unroll
  for (int i = 0; i < 4; ++i) { const real e = u[i] - ru[i]; t += e * cw.fR[m][i] * e; }
  l += t;
  l += real(0.0);  // S = 0 for the floating base (y = 0)
  return l * dt;
}

// Derivatives of a WB running cost w.r.t. u and the stance force (CostBase.cpp:19-34 and
// the CALC_PARTIALS_ONLY branch of SinglePhase.cpp:219-249; joint limits carry eps_ReB = 0
// and contribute exact zeros).  out = lu[4], luu[4] (diagonal), ly[2], lyy[4] where ly/lyy
// are the entries of the stance foot's force slots (zero in flight).
static __device__ __forceinline__ void wb_cost_uy_derivs(const CostParams& cw, int mode, real dt, const real* u,
                                         const real* y, bool reb, real delta, real eps_tq,
                                         real eps_grf, real* out) {
  const int m = mode - 1;
  const real tq = cw.tq_lim, mu = cw.mu;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    real lu = (2 * dt * cw.wR[m][c]) * (u[c] - real(0.0));
    real luu = 2 * dt * cw.wR[m][c];
    if (reb) {
      real B, Bz, Bzz;
      // constraint c: g = -u_c + tq (gu = -1); constraint 4 + c: g = u_c + tq (gu = +1)
      reduced_barrier(-real(1.0) * u[c] + tq, delta, &B, &Bz, &Bzz);
      lu += eps_tq * Bz * -real(1.0) * dt;
      luu += eps_tq * (-real(1.0) * Bzz * -real(1.0)) * dt;
      reduced_barrier(real(1.0) * u[c] + tq, delta, &B, &Bz, &Bzz);
      lu += eps_tq * Bz * real(1.0) * dt;
      luu += eps_tq * (real(1.0) * Bzz * real(1.0)) * dt;
    }
    out[c] = lu;
    out[4 + c] = luu;
  }
  out[8] = out[9] = out[10] = out[11] = out[12] = out[13] = real(0.0);
  if (mode == 1 || mode == 3) {
    const int o = mode == 1 ? 2 : 0;
    const real fx = mode == 1 ? y[2] : y[0], fz = mode == 1 ? y[3] : y[1];
    const real s0 = cw.wS[m][o], s1 = cw.wS[m][o + 1];
    real ly0 = (2 * dt * s0) * (fx - real(0.0));
    real ly1 = (2 * dt * s1) * (fz - kGRF);
    real l00 = 2 * dt * s0, l01 = real(0.0), l10 = real(0.0), l11 = 2 * dt * s1;
    if (reb) {
      const real rows[3][2] = {{0, 1}, {-1, mu}, {1, mu}};  // coefficients on (Fx, Fz)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        real B, Bz, Bzz;
        reduced_barrier(rows[i][0] * fx + rows[i][1] * fz + 0, delta, &B, &Bz, &Bzz);
        ly0 += eps_grf * Bz * rows[i][0] * dt;
        ly1 += eps_grf * Bz * rows[i][1] * dt;
        l00 += eps_grf * (rows[i][0] * Bzz * rows[i][0]) * dt;
        l01 += eps_grf * (rows[i][0] * Bzz * rows[i][1]) * dt;
        l10 += eps_grf * (rows[i][1] * Bzz * rows[i][0]) * dt;
        l11 += eps_grf * (rows[i][1] * Bzz * rows[i][1]) * dt;
      }
    }
    out[8] = ly0; out[9] = ly1;
    out[10] = l00; out[11] = l01; out[12] = l10; out[13] = l11;
  }
}

static __device__ void wb_term_ref(const Cmd& cm, int mode, real pos, real* rx) {
  MHPC_NO_FMA_F32
#pragma unroll
  for (int i = 0; i < 14; ++i) rx[i] = cXtermWB[mode - 1][i];
  rx[7] = cm.vel;
  rx[0] = pos;
}

static __device__ void fb_term_ref(const Cmd& cm, real pos, real* rx) {
  MHPC_NO_FMA_F32
  rx[0] = pos; rx[1] = cm.height; rx[2] = 0; rx[3] = cm.vel; rx[4] = 0; rx[5] = 0;
}

// Terminal cost of a WB phase (CostBase.cpp:37-47, SinglePhase.cpp:251-275): 0.5 e' Qf e at
// the terminal state x against the reference at position refT and, at the end of a touchdown
// phase (modes 2, 4), the constraint value *h and the AL term 50 ((sigma h / 2)^2 + lambda h)
// of phase p.  *h is written only there: the caller starts it at 0.  sigma and lambda are
// loaded inside the AL branch (st is not read otherwise); the caller adds the result to the
// phase value in its own contraction state.
static __device__ __forceinline__ acc wb_terminal_cost(const CostParams& cw, const Cmd& cm, int mode,
                                                       real refT, const real* x, bool AL_active,
                                                       const ProbState* st, int p, real* h) {
  MHPC_NO_FMA_COST
  real rx[14];
  wb_term_ref(cm, mode, refT, rx);
  acc Phi = 0;
  for (int i = 0; i < 14; ++i) { const real e = x[i] - rx[i]; Phi += e * cw.wQf[mode - 1][i] * e; }
  Phi = Phi * acc(0.5);
  if (ntc_of(mode, true)) {
    *h = mode == 2 ? wb_touchdown_value<kFront>(x) : wb_touchdown_value<kBack>(x);
    if (AL_active) {
      const acc sg = st->sigma[p], lam = st->lambda[p];
      const acc sh2 = sg * *h / 2;
      Phi += 50 * (sh2 * sh2 + lam * *h);
    }
  }
  return Phi;
}

// Terminal cost of an SRB phase (CostBase.cpp:37-47): 0.5 (x - xr)' Qf (x - xr)
static __device__ __forceinline__ acc fb_terminal_cost(const CostParams& cw, const Cmd& cm, int mode,
                                                       real refT, const real* x) {
  MHPC_NO_FMA_COST
  real rx[6];
  fb_term_ref(cm, refT, rx);
  acc Phi = 0;
  for (int i = 0; i < 6; ++i) { const real e = x[i] - rx[i]; Phi += e * cw.fQf[mode - 1][i] * e; }
  return Phi * acc(0.5);
}

// Phase transition after the terminal state of WB phase p (MultiPhaseDDP.cpp:351-379), when a
// phase follows: the impact map after a touchdown phase (modes 2, 4), then the projection of
// the 14 WB states to the 6 SRB states when the next phase is an SRB one.  (serial_rollout,
// mhpc_kernels.hip, spells the same steps out: it hands out the state between the two.)
static __device__ __forceinline__ void wb_phase_transition(const Layout& L, int p, real* x) {
  const int mode = L.mode[p];
  if (p + 1 < L.P) {
    if (mode == 2 || mode == 4) {
      real xp[14], lam[2];
      wb_impact<real>(x, mode == 2 ? kFront : kBack, xp, lam);
      for (int i = 0; i < 14; ++i) x[i] = xp[i];
    }
    if (p + 1 >= L.n_wb) {
      const real t0 = x[0], t1 = x[1], t2 = x[2], t7 = x[7], t8 = x[8], t9 = x[9];
      x[0] = t0; x[1] = t1; x[2] = t2; x[3] = t7; x[4] = t8; x[5] = t9;
    }
  }
}

// The knot loops keep the sin / cos constants in registers (SinCosK): VGPR copies, opaque to
// the compiler, so it keeps them live instead of rematerialising each with two s_mov per use.
// (A macro: through a function taking the struct by reference the line search's multiplies
// came out with their operands commuted -- equal results, but not the same kernel text.)
#ifndef MHPC_RO_VCONST
#define MHPC_RO_VCONST 1
#endif
#if MHPC_RO_VCONST && !defined(MHPC_FP32)
#define MHPC_PIN_VGPRS(K) \
  _Pragma("unroll") for (int i_ = 0; i_ < 15; ++i_) asm volatile("" : "+v"((K).c[i_]))
#else
#define MHPC_PIN_VGPRS(K) do { } while (0)
#endif

// FootholdPlanner::get_foothold_location (FootholdPlan.h:26-50), velcmd 1.5 / ground
// -0.404 hard-coded by the reference (MHPCLocomotion.cpp:25).
static __device__ void plan_foothold(const real* x0, real stance_time, int mode, real* f) {
  MHPC_NO_FMA_F32
  f[0] = f[1] = f[2] = f[3] = 0;
  if (mode == 1) {
    f[2] = (cos(x0[2]) * (-real(0.19)) + x0[0]) + real(1.5) * stance_time / 2;
    f[3] = -real(0.404);
  } else if (mode == 3) {
    f[0] = (cos(x0[2]) * real(0.19) + x0[0]) + real(1.5) * stance_time / 2;
    f[1] = -real(0.404);
  }
}


}  // namespace MHPC_NS
