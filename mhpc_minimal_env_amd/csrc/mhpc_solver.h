// Device-side data model of the batched HSDDP solve (shared by kernels and runtime).
//
// HBM layout (one handle = one batch of B problems; each problem has its own phase layout --
// gait schedule -- drawn from the handle's layout table, and problems sharing a layout form a
// group; every array is problem-major so each problem's records are contiguous and a wave's
// loads of one knot record are coalesced):
//   traj   [B][NSLOT][NK][KS]  x(<=14) u(4) y(4) per knot, KS = 24 doubles.  NSLOT =
//          n_cand + 1 rollout slots; state.nom_slot names the nominal trajectory and the
//          line-search candidates write the other slots (no copy on acceptance).  NK is the
//          per-problem knot stride: the largest knot count of the handle's layouts.
//   refpos [B][NK]             forward position reference (ReferenceGen.h:94-109); the
//          rest of the reference is constant per mode and computed in registers.
//   K      [B][NK][56], du [B][NK][4], G [B][NK][14]   CostToGoStruct outputs per knot.
//   par    [B][18][NK][9] + [B][NK][14] (NK * PS per problem, par_col / par_jac below)
//          dynamics Jacobians of the nominal trajectory: 18 tangent directions x (7 qddot
//          rows + 2 contact-force rows) per WB knot, column-block major, then the knots'
//          control/force cost derivatives incl. the ReB barrier (computed once per partials
//          pass, so the backward kernel evaluates no transcendental); SRB knots are
//          differentiated in registers by the backward kernel.
//   px     [B][P][196]         impact Jacobian Px (column-major) at the end of WB phases.
//   state  [B]                 ProbState (control flow + AL/ReB parameters).
//   grp    [G]                 group table: a group is a (layout, parameter set) pair in use
//          (mhpc_set_layouts x mhpc_set_param_sets) and its record holds the Layout and the
//          CostParams (read through the constant address space: scalar loads); a layout shared
//          by several sets is stored once per group.  gidx [B] the problems grouped (group g =
//          positions [go[g], go[g+1]) of gidx), lid [B] each problem's group.
//   cmd    [B][2]              user command (vel, height) of each problem (mhpc_set_commands),
//          indexed by problem number: it follows a problem through every regrouping.
//   opt    [MAXO]              option table: the distinct HSDDP_OPTION records in use
//          (mhpc_set_option_sets), oid [B] each problem's record, by problem number like cmd.
//          Options are no grouping dimension: a kernel reads its problem's record in the
//          per-problem control flow (line-search selection, AL update, iteration caps), per lane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mhpc_real.h"

#include "../../include/mhpc_capi.h"

// (plain g++ compiles this header too: mhpc_plan.h and its host check, tests/native)
#if defined(__HIPCC__)
#define MHPC_HOST_DEVICE __host__ __device__
#else
#define MHPC_HOST_DEVICE
#endif

namespace MHPC_NS {

constexpr int KS = 24;        // doubles per knot record in traj
constexpr int PS_JAC = 162;   // 18 tangent directions x (7 qddot + 2 contact-force rows)
constexpr int PS = 176;       // doubles per knot in par: Jacobians + 14 cost derivatives
                              // (lu 4, luu 4, ly 2, lyy 4 of the stance block)
// par, per problem (NK = the knot stride, sp.NK): 18 column blocks [NK][9] -- column c of
// knot k at (c NK + k) 9 -- then the cost derivatives [NK][14].  A direction's values of
// consecutive knots are contiguous, so the partials' lanes (consecutive knots) store whole
// lines; the sweep's lane walks its own column block backwards, one 72-byte piece per knot.
MHPC_HOST_DEVICE inline size_t par_col(int NK, int b, int c, int kk) {
  return (size_t)b * NK * PS + ((size_t)c * NK + kk) * 9;
}
MHPC_HOST_DEVICE inline size_t par_jac(int NK, int b, int kk) {
  return (size_t)b * NK * PS + (size_t)PS_JAC * NK + (size_t)kk * 14;
}
constexpr int MAXP = MHPC_MAX_PHASES;
constexpr int MAXC = 32;      // max line-search candidates
constexpr int MAXL = MHPC_MAX_LAYOUTS;  // distinct phase layouts per handle
constexpr int MAXO = MHPC_MAX_OPTION_SETS;  // distinct option records per handle
constexpr int ST_RMAX = 128;  // line search: staged position references per problem (knots per phase)
constexpr int TRACE = MHPC_TRACE_LEN;

// Counter slots of ProbState::cnt.  C_LS is the reference-equivalent number of serial
// line-search rollouts; C_*_RUN count what this implementation actually executed; the
// knot / Px counters feed the algorithmic-byte model of the roofline report.
enum {
  C_DDP = 0, C_BWS, C_BWS_KNOTS, C_LS, C_FWD, C_PAR, C_LS_RUN, C_PAR_RUN,
  C_LS_LAUNCH, C_BWS_KNOTS_WB, C_BWS_KNOTS_FB, C_PX_READS,
  C_BWS_KNOTS_FB1,  // SRB knots swept by the SRB half of a split sweep (its first attempt)
  NCNT
};

// Cost weights (diagonals per mode, CostBase.h:9-46 / MHPCCost.cpp:24-75) and constraint
// parameters (ConstraintsBase.h:11-50 / MHPCConstraints.cpp:14-88) of one parameter set:
// mhpc_set_cost_weights / mhpc_set_constraint_params / mhpc_set_param_sets; every kernel reads
// its block's group record DevBufs::grp[g].cw (params_of, mhpc_device.h).
struct CostParams {
  real wQ[4][14], wR[4][4], wS[4][4], wQf[4][14];  // whole-body phases
  real fQ[4][6], fR[4][4], fQf[4][6];              // SRB phases
  real tq_lim, mu;                                 // torque limit, GRF friction coefficient
  real sigma0[4], delta0[4], delta_min[4], eps_tq0[4], eps_grf0[4];  // AL / ReB initial values
};

// Phase layout of one group of problems (MHPCLocomotion::build_problem, MHPCLocomotion.cpp
// :63-104, for that problem's gait point): n_wb whole-body phases, then SRB phases.
struct Layout {
  int P, n_wb, NK;          // phases, whole-body phases, knots of this layout (<= SolveParams::NK)
  int mode[MAXP], N[MAXP], ko[MAXP], xs[MAXP];
  int buf[MAXP];            // phase buffer of each phase (receding horizon, see k_store_*)
  // partials work per problem and its prefix offsets per phase: WB knots with Jacobians
  // (N - 1 per WB phase) and impact directions (14 per touchdown phase)
  int par_knots, par_imp;
  int par_knot_off[MAXP + 1], par_imp_off[MAXP + 1];
  real dt[MAXP];
};

// Record of one group: its layout and its parameter set, side by side, so that a kernel
// addresses both from one base (one scalar register pair live through its loops, as before
// parameter sets -- the sweep and the line search have no scalar registers to spare).
struct Group {
  Layout lay;
  CostParams cw;
};

struct SolveParams {
  int B;                   // problems of the handle (the arrays' leading dimension)
  int NK;                  // per-problem knot stride of the packed arrays (max over layouts)
  // groups: the problems of group g are gidx[go[g] .. go[g + 1]) and share the group record
  // grp[g] (layout and parameter set); a launch enumerates its blocks group by group, so no
  // block mixes layouts or parameter sets (kernels map a block to its group with block_group,
  // mhpc_device.h).  ident: gidx is the identity.
  int ngrp, ident;
  int go[MAXL + 1];
  int gpk[MAXL], gpi[MAXL];  // partials knot / impact work items per problem of each group
  int pmax;                  // most phases of any layout
  int n_cand, nslot;
  real eps[MAXC];          // line-search grid 1, alpha, alpha^2, ... (host libm)
  real eps9;               // pow(0.1, 9) (SinglePhase.cpp:202), host libm
  // problem 0's update_penalty and ReB_active: only k_init reads them, for the option state it
  // writes for every problem; the problems' own values then come from the option table
  // (k_init_params, which says why k_init keeps reading this block).  Every other kernel reads
  // the problem's record DevBufs::opt[oid[b]] alone.
  real update_penalty;
  int ReB_active;
  // What the problems of a solve's scope have in common (scope_caps, mhpc_plan.h; set in the
  // scope's copy of this block): the smallest iteration caps among them -- an op within both takes
  // every problem, so its kernels skip the per-problem gate and its two dependent loads -- and
  // their AL_active when they all agree (-1: they differ, read the record).  With one option set
  // no kernel of the schedule reads the table before the line search's selection.
  int min_n_al, min_max_ddp, al_uniform;
  // launch shape (host side only): compute units of the handle's device and the kernel
  // variants forced through mhpc_set_kernel_variant (0 = chosen by batch size)
  int ncu, var_bws, var_ro, var_overlap;
  // line-search trials that store their running knot records (the first ro_store, and the
  // last; the rest are rolled out again when accepted -- mhpc_kernels.hip RO_STORE_FIRST)
  int ro_store;
  // host side: some layout has both kinds of phase (the sweep can run split, bws_split) /
  // every phase of every layout fits the line search's LDS stage of position references
  int split_ok, stage_fits;
  // problem 0's parameter set (what mhpc_get_cost_weights / mhpc_get_constraint_params report).
  // Only k_init reads it, for the AL / ReB initial values it writes for every problem; the
  // groups' own values then come from the table (k_init_params, mhpc_init.hip, which says
  // why k_init keeps this read).  Every other kernel reads the group table alone.
  CostParams cw;
};

// User command of one problem (the reference's MHPCUserParameters::usrcmd of one controller,
// handed to ReferenceGen by build_problem, MHPCLocomotion.cpp:98-103): DevBufs::cmd[b].
struct Cmd {
  real vel, height;
};

// One option record (MultiPhaseDDP::_option of one controller, MHPC_CompoundTypes.h:196-212) as the
// kernels read it: the fields of mhpc_hsddp_option but alpha (the handle's line-search grid) and
// smooth_active (carried on the host only), and the integer iteration caps the launch schedule
// is sized with (option_cap, mhpc_plan.h): the problem takes part in op (al, ddp) of a schedule
// only while al <= n_al and ddp <= max_ddp.
struct OptRec {
  real gamma, DDP_thresh, AL_thresh, update_penalty, update_relax, update_regularization,
      update_ReB;
  int32_t AL_active, ReB_active;
  int32_t n_al, max_ddp;
};

// Costs, their sums and the expected cost change are accumulated and compared in fp64 in
// both builds (the fp32 build keeps its dynamics, partials and sweep in fp32): a total cost
// of ~1e5 summed over ~700 knots in fp32 carries errors of the size of the Armijo margins.
using acc = double;

struct ProbState {
  acc J, viol, dV_exp;
  real reg;
  acc cost_prev;
  acc V[MAXP], dV[MAXP];
  real h[MAXP];
  real sigma[MAXP], lambda[MAXP], delta[MAXP], eps_tq[MAXP], eps_grf[MAXP];
  int32_t status;      // mhpc_solve_status
  int32_t active;      // still inside the AL loop
  int32_t ddp_active;  // still inside the DDP loop of this AL iteration
  int32_t reb_active;  // _option.ReB_active of this AL iteration
  int32_t al_partials; // terminal AL partials present (B1: only after forward_sweep(0))
  int32_t nom_slot;
  int32_t al_iter, ddp_iter;
  int32_t bws_iter;    // backward sweeps of this DDP iteration
  int32_t ntrace;
  int32_t trace[TRACE];
  int64_t cnt[NCNT];
  // state of the last running/terminal-cost partials evaluation (forward_sweep(0) or
  // forward_sweep_partials_only) for print_debugInfo's cost.txt: the nominal slot it saw,
  // whether the AL terms entered Phix (B1) and the sigma / lambda it used
  int32_t par_slot, par_al;
  real par_sigma[MAXP], par_lambda[MAXP];
  // line-search trials run after that evaluation (only the final, converged line search of
  // an AL iteration): the reference's dynamics-only sweeps add their AL terms to Phix too
  // (guard quirk of SinglePhase.cpp:269), which cost.txt shows.  Trial j lives in slot
  // j < ls_nom ? j : j + 1.
  int32_t ls_nt, ls_nom;
  real ls_sigma[MAXP], ls_lambda[MAXP];
  // line-search trial whose running records were not stored (trials j >= RO_STORE_FIRST but
  // the last, mhpc_kernels.hip) and must be rolled out again into its slot, -1 if none; the
  // nominal slot that line search started from
  int32_t reroll_j, reroll_nom;
  real reroll_eps;  // its step size (eps of trial reroll_j)
  // MultiPhaseDDP::_option as solve() leaves it: ReB_active and update_penalty are rewritten
  // inside the AL loop (MultiPhaseDDP.cpp:178-183, 273-277) and the next solve() starts from
  // the rewritten values (captured at its first AL iteration: cap_*) -- visible across the
  // solves of a receding-horizon loop.  mhpc_initialize restores the problem's own option record.
  int32_t opt_reb, cap_reb;
  real opt_pen, cap_pen;
};

// Value function where the backward sweep crosses from the SRB phases into the WB phases
// (the sweep runs as two launches when the SRB part overlaps the partials):
// H / G of knot 0 of phase n_wb (row stride NX of that phase) from the first attempt whose
// SRB part passed the PSD test -- the SRB half retries attempts that fail there itself --,
// that attempt's regularisation and number (bws_iter), whether the retries aborted
// (regularisation > 1000), the attempts and SRB knots swept.
struct BwsCarry {  // double in both builds: the sweep's arithmetic type (mhpc_bws.hip breal)
  double H[196];
  double G[14];
  double reg;
  int32_t abort, iter, sweeps, knots;
};

struct DevBufs {
  real* traj;
  real* refpos;
  real* K;
  real* du;
  real* G;
  real* par;
  real* px;
  real* x0;
  ProbState* st;
  real* out;    // export staging [B][NK][KS]
  BwsCarry* carry;  // [B]
  const Group* grp;   // [ngrp] group table: layout and parameter record of each group
  const int* gidx;    // [B] problems grouped (by layout, then parameter set)
  const int* lid;     // [B] group of each problem (its record grp[lid[b]])
  const Cmd* cmd;     // [B] user command of each problem
  const OptRec* opt;  // [MAXO] option table
  const int* oid;     // [B] option record of each problem (opt[oid[b]])
};

}  // namespace MHPC_NS
