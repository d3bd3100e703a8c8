// Host runtime behind include/mhpc_capi.h: handle lifetime, HBM allocation, and the
// fixed kernel schedule of one batched solve (MultiPhaseDDP::solve restated as launches
// over a device-resident per-problem state machine).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/mhpc_capi.h"
#include "mhpc_devres.h"
#include "mhpc_devtemp.h"
#include "mhpc_launch.h"
#include "mhpc_plan.h"
#include "mhpc_snapshot_map.h"
#include "mhpc_step_map.h"

extern thread_local std::string mhpc_g_err;  // mhpc_capi.cpp (mhpc_last_error)

#define API_NS MHPC_NS
#include "mhpc_api_decl.h"
#undef API_NS

namespace MHPC_NS {
namespace {
int fail(int code, const std::string& msg) {
  mhpc_g_err = msg;
  return code;
}
// The epilogue of a failed call: undo() (a rollback, which may fail in turn) with the failure's
// own message kept; drain: the given streams, in that order, so that nothing of the handle's stays
// queued behind the failure.
template <class Undo>
void keep_error(Undo undo) {
  const std::string why = mhpc_g_err;
  undo();
  mhpc_g_err = why;
}
void drain(std::initializer_list<hipStream_t> streams) {
  keep_error([&] {
    for (hipStream_t q : streams) (void)hipStreamSynchronize(q);
  });
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(MHPC_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
// a check or planner of mhpc_plan.h (its trailing argument the message): a refusal goes to fail()
#define PLANCHK(call, ...)                                 \
  do {                                                     \
    const char* msg_ = nullptr;                            \
    if (int rc_ = call(__VA_ARGS__, &msg_)) return fail(rc_, msg_); \
  } while (0)
}  // namespace

enum { K_INIT = 0, K_FULL, K_LS, K_PAR, K_BWS, K_AL, K_BWS_SRB, NKERN };
static const char* kKernelNames[NKERN] = {"k_init", "k_cost(forward_sweep0)", "k_rollout(linesearch)",
                                          "k_partials", "k_bws", "k_al_end", "k_bws_srb"};

struct Handle {
  // What the handle owns on the device (mhpc_devres.h), mirrored by tests/native/devres_hostcheck.cpp.
  // ~Handle releases from the last member to the first, and that order is kept: device memory
  // first (mhpc_destroy has drained every stream), in the order the arrays were always freed; then
  // the events, each before the streams it was recorded on; the main stream last.
  StreamSet main;  // s1: the handle's stream; the partials run on s2 / s3 beside the SRB sweep
  Event evstart;   // sub-batches (MHPC_VARIANT_SUBBATCH): each block on a set of its own (first use)
  std::vector<StreamSet> subs;
  Event ev0, ev1;
  std::vector<Event> evpool;  // profiling: one event pair per launch of a solve (evkind)
  // at first use: the event that orders the handle's stream behind a caller's (control I/O), and
  // those around a whole mhpc_tick_problems (ev0 / ev1 bracket its solve schedule)
  Event evctl, evt0, evt1;
  // the control steps [B] (first call with steps), the split order [B] of a mixed first op, the
  // buffer store [B][spmax][nbk] (first update), the reduced counters per group [MAXL][NCNT]
  DevArray<int> dstep, dsplit;
  DevArray<real> store;
  DevArray<unsigned long long> dcnt;
  struct Arrays {  // behind the views of d (set_views)
    DevArray<int> oid;
    DevArray<OptRec> opt;  // [MAXO]
    DevArray<Cmd> cmd;
    DevArray<int> lid, gidx;
    DevArray<Group> grp;  // [MAXL]
    DevArray<BwsCarry> carry;
    DevArray<real> out;
    DevArray<ProbState> st;
    DevArray<real> x0, px, par, G, du, K, refpos, traj;
  } own;

  mhpc_problem_desc desc;  // the descriptor of mhpc_create (precision, vel, height)
  mhpc_hsddp_option opt;   // the option of mhpc_create: its alpha is the handle's line-search grid
  // option sets (mhpc_set_option_sets): the table of distinct records in use with each problem's
  // slot by problem number (mhpc_plan.h, OptTable); the device copies own.opt and own.oid.
  // otab.rec[otab.of[0]] is what mhpc_get_options reports.
  OptTable otab;
  int device = 0;
  SolveParams sp;
  DevBufs d;  // the arrays as the kernels receive them: views of `own`
  bool x0_set = false, initialized = false, solved = false, x0_changed = false;
  // constraint parameters replaced after the last initialize / update_problem: their AL / ReB
  // initial values reach the problems' state only there, so a solve in between
  // would mix new limits with old initial values -- refused until then
  bool params_changed = false;
  // per-problem user commands [B] (vel, height) as the caller gave them (the device copy is
  // cast to real), indexed by problem number.  A problem whose command changed after its references
  // were last generated is marked in the ledger: the position references still belong to the old
  // speed, so a solve in between is refused like one after new constraint parameters
  std::vector<double> cmd;
  // per-problem call-order state (mhpc_plan.h, Ledger): fresh, open SRB nominal, command mark
  Ledger led;
  // parameter sets (mhpc_set_param_sets): the distinct sets in use, as the kernels read them
  // (real), and each problem's set by problem number; psets[pset_of[0]] is what the handle-wide
  // getters report.  sets_changed: a mixed call changed some problem's values on an initialised
  // handle (set together with params_changed; mhpc_rollout_costs looks at this one alone)
  std::vector<CostParams> psets;
  std::vector<int> pset_of;
  bool sets_changed = false;
  float solve_ms = 0;
  unsigned long long cnt[NCNT] = {};  // the reduced counters' sum over the groups
  unsigned long long gcnt[MAXL][NCNT] = {};
  // profiling: the event pairs of evpool, accumulated per kernel id
  bool profile = false;
  std::vector<int> evkind;
  double kms[NKERN] = {}, kbytes[NKERN] = {}, kflops[NKERN] = {};
  int64_t klaunch[NKERN] = {};
  // per-problem layouts, and the plan installed from them and the parameter sets (plan_groups,
  // mhpc_plan.h; commit_groups): each group's layout, descriptor, byte model and set, each
  // problem's group, the problems grouped.  The device copies: own.grp, own.lid, own.gidx.
  std::vector<ProbLayout> pl;
  GroupPlan plan;
  // receding horizon (MHPCLocomotion::update_problem): each problem's current mode, the
  // shape of the buffer store, knot capacity of the packed arrays, and whether the next solve's
  // first forward_sweep(0) must be a real rollout (rotated nominal, new x0)
  std::vector<int> cmode;
  int nbk = 0, nk_cap = 0, spmax = 0;
  int nk_floor = 0;  // mhpc_reserve_knots: floor of the knot stride wherever it may change
  bool need_full = false;
  bool store_valid = false;  // store zeroed since the last initialize (memory_reset)
  // (dsplit: the grouped order of a solve that starts with the real rollout (need_full) while the
  // ledger has fresh problems, split for its first op: the others first, then the fresh ones)
  int nsub_req = 0;  // MHPC_VARIANT_SUBBATCH: the schedule runs once per contiguous block of problems
  int ro_store_req = 0;  // MHPC_VARIANT_RO_STORE (0: by the batch's line-search shape)
  int sweep_bits = 0;    // MHPC_VARIANT_SWEEP_BITS (0 = 64: the sweep computes in double)
  int snap_round_req = 0;  // MHPC_VARIANT_SNAP_ROUND (0: as many problems as fit the staging cap)
  std::vector<int> hstep;  // the host copy of dstep that its upload reads
};

// backward sweep: per WB knot partials record + x,u,y + refpos read, K,du,G written;
// per SRB knot x,u + refpos read, K,du,G written; Px read per impact-aware step
static constexpr double kBwsWbKnot = kB * (PS + 22 + 1 + 56 + 4 + 14);
static constexpr double kBwsFbKnot = kB * (10 + 1 + 24 + 4 + 6);
static constexpr double kBwsPx = kB * 196;
// Algorithmic FP64 flops of the backward sweep in the reference's dense formulation
// (compute_Qfunction 20.2k + valuefunction_update 4.3k per WB knot,
// ~3k per SRB knot; impact_aware_step Px' G, Px' H Px: 2 (2 * 14^3) + 2 * 14^2).  The
// kernel skips the structural zeros, so this is the dense-equivalent rate, an upper bound
// on the flops it executes.
static constexpr double kFlopWbKnot = 24.5e3, kFlopFbKnot = 3.0e3,
                        kFlopPx = 2.0 * (2.0 * 14 * 14 * 14) + 2.0 * 14 * 14;

const char* api_kernel_name(int k) {
  return (k >= 0 && k < NKERN) ? kKernelNames[k] : "";
}


// The one place where d gets its pointers: called wherever an array of `own` is (re)allocated.
static void set_views(Handle* h) {
  const Handle::Arrays& a = h->own;
  h->d = DevBufs{a.traj.get(), a.refpos.get(), a.K.get(),    a.du.get(),   a.G.get(),   a.par.get(),
                 a.px.get(),   a.x0.get(),     a.st.get(),   a.out.get(),  a.carry.get(), a.grp.get(),
                 a.gidx.get(), a.lid.get(),    a.cmd.get(),  a.opt.get(),  a.oid.get()};
}
// Every stream of the handle drained, the main set and each sub-batch's; the first error.
static hipError_t sync_streams(const Handle* h) {
  hipError_t e = h->main.sync();
  for (const StreamSet& s : h->subs) {
    const hipError_t e1 = s.sync();
    if (e == hipSuccess) e = e1;
  }
  return e;
}

// The packed per-knot arrays for a knot stride of NK (grown, never shrunk: their content is
// rebuilt by initialize / update_problem).  The partials records' zero columns (x, z, xdot,
// zdot) are written by no kernel: they are zeroed here whenever the stride changes, since the
// column blocks are stride-major (par_col) and a new stride moves them onto words the old
// stride used for other columns.  New arrays are allocated before the old ones are freed, so
// a failed allocation leaves the handle's arrays and stride as they were.
static int ensure_knot_arrays(Handle* h, int NK) {
  const DevBufs& d = h->d;
  const size_t B = h->sp.B, nk = NK;
  const bool grow = NK > h->nk_cap;
  if (!grow && NK == h->sp.NK) return MHPC_OK;
  HIPCHK(sync_streams(h));
  if (grow) {
    Handle::Arrays& a = h->own;
    DevArray<real>* const arr[] = {&a.traj, &a.refpos, &a.K, &a.du, &a.G, &a.par, &a.out};
    const size_t n = B * nk;
    const size_t count[] = {n * h->sp.nslot * KS, n, n * 56, n * 4, n * 14, n * PS, n * KS};
    if (const hipError_t e = grow_and_swap(arr, count))
      return fail(MHPC_ERR_DEVICE, std::string("knot array allocation failed: ") + hipGetErrorString(e));
    set_views(h);
    h->nk_cap = NK;
    HIPCHK(hipMemsetAsync(d.traj, 0, B * h->sp.nslot * nk * KS * sizeof(real), h->main.s1));
  }
  HIPCHK(hipMemsetAsync(d.par, 0, B * nk * PS * sizeof(real), h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}

// The group table (group g: layout lays[g], parameter set gset[g]) to the device.
static int upload_params(Handle* h) {
  std::vector<Group> t(h->plan.gset.size());
  for (size_t g = 0; g < t.size(); ++g) t[g] = Group{h->plan.lays[g], h->psets[h->plan.gset[g]]};
  h->sp.cw = h->psets[h->pset_of[0]];  // k_init's copy (problem 0's set)
  HIPCHK(hipMemcpyAsync(h->own.grp.get(), t.data(), t.size() * sizeof(Group), hipMemcpyHostToDevice,
                        h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}

// The installed plan's grouped order, each problem's group and the group table to the device.
static int upload_plan(Handle* h) {
  const size_t B = h->sp.B;
  HIPCHK(hipMemcpyAsync(h->own.gidx.get(), h->plan.gidx.data(), B * sizeof(int), hipMemcpyHostToDevice, h->main.s1));
  HIPCHK(hipMemcpyAsync(h->own.lid.get(), h->plan.lid.data(), B * sizeof(int), hipMemcpyHostToDevice, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return upload_params(h);
}

// k_init's copy of problem 0's option record (SolveParams::update_penalty / ReB_active)
static void mirror_option0(Handle* h) {
  const OptRec r0 = option_record(h->otab.rec[h->otab.of[0]]);
  h->sp.update_penalty = r0.update_penalty;
  h->sp.ReB_active = r0.ReB_active;
}
// The option table to the device (every slot; a free one holds a stale record nobody indexes), and
// k_init's copy of problem 0's record.
static int upload_options(Handle* h) {
  std::vector<OptRec> t(h->otab.rec.size());
  for (size_t s = 0; s < t.size(); ++s) t[s] = option_record(h->otab.rec[s]);
  mirror_option0(h);
  HIPCHK(hipMemcpyAsync(h->own.opt.get(), t.data(), t.size() * sizeof(OptRec), hipMemcpyHostToDevice, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}
// More than one parameter set or option set: k_init wrote problem 0's values for every problem and
// k_init_params must follow it with each problem's own.
// The same kernel leaves the SRB nominal of a problem without AL iterations open (zero, as the
// reference's), so a single record with no AL iteration needs it too.
static bool no_al_iteration(const mhpc_hsddp_option& o) { return option_cap(o.max_AL_iter) == 0; }
static bool own_init_values(const Handle* h) {
  if (h->psets.size() > 1 || h->otab.in_use() > 1) return true;
  return no_al_iteration(h->otab.rec[h->otab.of[0]]);
}

// The one way a new grouping reaches a handle: `plan` (plan_groups over the new layouts and sets)
// and whichever of the per-problem layouts, the parameter sets and the problems' sets it was
// planned from that differ from the handle's (null: the handle's own).  Grows or re-strides the
// packed arrays for the plan's longest layout, installs the plan with the launch fields of sp, and
// uploads the grouped order and the group table.  keep_stride (mhpc_reset_problems and
// mhpc_copy_problems, whose layouts were checked to fit, and the parameter-set calls, which change
// no layout): the knot stride stays what it is even if the longest layout left, so no array is
// re-strided, re-zeroed or reallocated and the problems' records stay where they are.
// Everything is swapped in: after MHPC_OK the arguments hold what the handle held before (commit
// them again to go back, as mhpc_copy_problems does).  On an error nothing has changed: a failed
// allocation leaves the arrays as they were, and after a failed upload the previous plan, layouts,
// sets and stride are put back here, host and device (as far as the device still answers).
static int commit_groups(Handle* h, GroupPlan&& plan, bool keep_stride,
                         std::vector<ProbLayout>* pl = nullptr, std::vector<CostParams>* psets = nullptr,
                         std::vector<int>* pset_of = nullptr) {
  const int old_NK = h->sp.NK;
  if (!keep_stride) {  // the longest layout, or the floor of mhpc_reserve_knots
    const int NK = std::max(plan.NK, h->nk_floor);
    if (int rc = ensure_knot_arrays(h, NK)) return rc;
    h->sp.NK = NK;
  }
  auto exchange = [&] {
    std::swap(h->plan, plan);
    if (pl) h->pl.swap(*pl);
    if (psets) h->psets.swap(*psets);
    if (pset_of) h->pset_of.swap(*pset_of);
    h->plan.to_params(h->sp);
  };
  exchange();
  const int rc = upload_plan(h);
  if (rc)
    keep_error([&] {
      exchange();
      if (h->sp.NK != old_NK && ensure_knot_arrays(h, old_NK) == MHPC_OK) h->sp.NK = old_NK;
      if (!h->plan.gidx.empty()) (void)upload_plan(h);  // (mhpc_create has no previous plan)
    });
  return rc;
}

// Host (double) parameter structs <-> the kernels' parameter block (real).
static void put_weights(CostParams& cw, const mhpc_cost_weights& w) {
  for (int m = 0; m < 4; ++m) {
    for (int i = 0; i < 14; ++i) {
      cw.wQ[m][i] = (real)w.wb_Q[m][i];
      cw.wQf[m][i] = (real)w.wb_Qf[m][i];
    }
    for (int i = 0; i < 4; ++i) {
      cw.wR[m][i] = (real)w.wb_R[m][i];
      cw.wS[m][i] = (real)w.wb_S[m][i];
      cw.fR[m][i] = (real)w.fb_R[m][i];
    }
    for (int i = 0; i < 6; ++i) {
      cw.fQ[m][i] = (real)w.fb_Q[m][i];
      cw.fQf[m][i] = (real)w.fb_Qf[m][i];
    }
  }
}
static void get_weights(const CostParams& cw, mhpc_cost_weights& w) {
  for (int m = 0; m < 4; ++m) {
    for (int i = 0; i < 14; ++i) {
      w.wb_Q[m][i] = cw.wQ[m][i];
      w.wb_Qf[m][i] = cw.wQf[m][i];
    }
    for (int i = 0; i < 4; ++i) {
      w.wb_R[m][i] = cw.wR[m][i];
      w.wb_S[m][i] = cw.wS[m][i];
      w.fb_R[m][i] = cw.fR[m][i];
    }
    for (int i = 0; i < 6; ++i) {
      w.fb_Q[m][i] = cw.fQ[m][i];
      w.fb_Qf[m][i] = cw.fQf[m][i];
    }
  }
}
static void put_constraints(CostParams& cw, const mhpc_constraint_params& c) {
  cw.tq_lim = (real)c.torque_limit;
  cw.mu = (real)c.friction_coeff;
  for (int m = 0; m < 4; ++m) {
    cw.sigma0[m] = (real)c.sigma[m];
    cw.delta0[m] = (real)c.delta[m];
    cw.delta_min[m] = (real)c.delta_min[m];
    cw.eps_tq0[m] = (real)c.eps_torque[m];
    cw.eps_grf0[m] = (real)c.eps_grf[m];
  }
}
static void get_constraints(const CostParams& cw, mhpc_constraint_params& c) {
  c.torque_limit = cw.tq_lim;
  c.friction_coeff = cw.mu;
  for (int m = 0; m < 4; ++m) {
    c.sigma[m] = cw.sigma0[m];
    c.delta[m] = cw.delta0[m];
    c.delta_min[m] = cw.delta_min[m];
    c.eps_torque[m] = cw.eps_tq0[m];
    c.eps_grf[m] = cw.eps_grf0[m];
  }
}

static int check_weights(const mhpc_cost_weights* w) {
  const double* v = &w->wb_Q[0][0];
  for (size_t i = 0; i < sizeof(mhpc_cost_weights) / sizeof(double); ++i)
    if (!std::isfinite(v[i]) || v[i] < 0) return fail(MHPC_ERR_INVALID, "cost weights must be finite and >= 0");
  return MHPC_OK;
}
static int check_constraints(const mhpc_constraint_params* c) {
  const double* v = &c->torque_limit;
  for (size_t i = 0; i < sizeof(mhpc_constraint_params) / sizeof(double); ++i)
    if (!std::isfinite(v[i])) return fail(MHPC_ERR_INVALID, "constraint parameters must be finite");
  if (!(c->torque_limit > 0)) return fail(MHPC_ERR_INVALID, "torque_limit must be > 0");
  if (!(c->friction_coeff >= 0))
    return fail(MHPC_ERR_INVALID, "friction_coeff must be >= 0 (a negative one inverts the GRF cone)");
  for (int m = 0; m < 4; ++m) {
    if (!(c->delta[m] > 0) || !(c->delta_min[m] > 0))
      return fail(MHPC_ERR_INVALID, "delta and delta_min must be > 0");
    if (c->delta_min[m] > c->delta[m])
      return fail(MHPC_ERR_INVALID, "delta_min must not exceed delta (the AL update only shrinks delta)");
    if (c->sigma[m] < 0 || c->eps_torque[m] < 0 || c->eps_grf[m] < 0)
      return fail(MHPC_ERR_INVALID, "sigma and the ReB weights must be >= 0");
  }
  return MHPC_OK;
}

// A handle-wide setter rewrote one half of every set in `ns`: sets that became equal merge (the
// groups are then rebuilt), otherwise only the device table changes.  On a device error the
// handle keeps its old sets, host and device (as far as the device still answers).
static int apply_sets(Handle* h, std::vector<CostParams>& ns) {
  HIPCHK(hipSetDevice(h->device));
  std::vector<int> nof = h->pset_of;
  const size_t n = ns.size();
  merge_sets(ns, nof);
  if (ns.size() == n) {  // nothing merged: the same groups with new values
    h->psets.swap(ns);
    const int rc = upload_params(h);
    if (rc) {
      h->psets.swap(ns);
      (void)upload_params(h);
    }
    return rc;
  }
  GroupPlan plan;
  PLANCHK(plan_groups, h->pl, nof, plan);
  // (no layout changes here: the knot stride stays, also one a reset left above the longest layout)
  return commit_groups(h, std::move(plan), true, nullptr, &ns, &nof);
}

int api_set_cost_weights(Handle* h, const mhpc_cost_weights* w) {
  if (!h || !w) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = check_weights(w);
  if (rc) return rc;
  std::vector<CostParams> ns = h->psets;
  for (CostParams& cw : ns) put_weights(cw, *w);
  return apply_sets(h, ns);
}
int api_get_cost_weights(Handle* h, mhpc_cost_weights* w) {
  if (!h || !w) return fail(MHPC_ERR_INVALID, "null argument");
  get_weights(h->psets[h->pset_of[0]], *w);
  return MHPC_OK;
}
int api_set_constraint_params(Handle* h, const mhpc_constraint_params* c) {
  if (!h || !c) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = check_constraints(c);
  if (rc) return rc;
  std::vector<CostParams> ns = h->psets;
  for (CostParams& cw : ns) put_constraints(cw, *c);
  if ((rc = apply_sets(h, ns))) return rc;
  if (h->initialized) h->params_changed = true;
  return MHPC_OK;
}
int api_get_constraint_params(Handle* h, mhpc_constraint_params* c) {
  if (!h || !c) return fail(MHPC_ERR_INVALID, "null argument");
  get_constraints(h->psets[h->pset_of[0]], *c);
  return MHPC_OK;
}

// Per-problem parameter sets (the batch axis over WBCost / FBCost / WBConstraint objects):
// problem b gets w[set_of[b]] / c[set_of[b]] on top of problem 0's current values for the half
// not given.  Equal sets merge, unused ones are dropped, and the groups are rebuilt over the
// (layout, set) pairs; a call that changes no problem's values changes nothing.
int api_set_param_sets(Handle* h, int n_sets, const mhpc_cost_weights* w,
                       const mhpc_constraint_params* c, const int32_t* set_of) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (n_sets < 1 || n_sets > MHPC_MAX_PARAM_SETS)
    return fail(MHPC_ERR_INVALID, "n_sets must be 1..MHPC_MAX_PARAM_SETS");
  int rc;
  for (int i = 0; i < n_sets; ++i) {
    if (w && (rc = check_weights(&w[i]))) return rc;
    if (c && (rc = check_constraints(&c[i]))) return rc;
  }
  const int B = h->sp.B;
  for (int b = 0; set_of && b < B; ++b)
    if (set_of[b] < 0 || set_of[b] >= n_sets) return fail(MHPC_ERR_INVALID, "set index out of range");
  std::vector<CostParams> ns(n_sets, h->psets[h->pset_of[0]]);
  for (int i = 0; i < n_sets; ++i) {
    if (w) put_weights(ns[i], w[i]);
    if (c) put_constraints(ns[i], c[i]);
  }
  std::vector<int> nof(B);
  for (int b = 0; b < B; ++b) nof[b] = set_of ? set_of[b] : b % n_sets;
  merge_sets(ns, nof);
  bool changed = false;
  for (int b = 0; b < B && !changed; ++b)
    changed = !same_params(ns[nof[b]], h->psets[h->pset_of[b]]);
  if (!changed) return MHPC_OK;  // nothing changes: nothing pending
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  GroupPlan plan;
  PLANCHK(plan_groups, h->pl, nof, plan);  // too many (layout, set) pairs: the old sets stay
  // (the knot stride stays as in apply_sets: the records of an initialised handle are live)
  if ((rc = commit_groups(h, std::move(plan), true, nullptr, &ns, &nof))) return rc;
  if (h->initialized) h->params_changed = h->sets_changed = true;
  return MHPC_OK;
}
int api_get_problem_params(Handle* h, int b, mhpc_cost_weights* w, mhpc_constraint_params* c) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (b < 0 || b >= h->sp.B) return fail(MHPC_ERR_INVALID, "problem out of range");
  if (w) get_weights(h->psets[h->pset_of[b]], *w);
  if (c) get_constraints(h->psets[h->pset_of[b]], *c);
  return MHPC_OK;
}
int api_num_param_sets(Handle* h, int* n) {
  if (!h || !n) return fail(MHPC_ERR_INVALID, "null argument");
  *n = (int)h->psets.size();
  return MHPC_OK;
}

static int dev_fail(const char* fn, hipError_t e);

// ---- per-problem option sets (mhpc_set_option_sets) ---------------------------------------------
// In the reference each MHPCLocomotion owns its MultiPhaseDDP::_option, and giving a controller
// another option is `_option = o`.  Here: validate every record, plan the table on a working copy
// (plan_options, mhpc_plan.h), and only then upload the table and run the list-driven kernel over
// the problems whose record changed (their oid entry, and the two fields a solve rewrites).  A
// problem whose record did not change keeps its slot and its device state; a call that changes no
// problem touches nothing.  Nothing becomes pending: the next solve or tick reads the new records.
int api_set_option_sets(Handle* h, int n_sets, const mhpc_hsddp_option* sets, const int32_t* set_of) {
  if (!h || !sets) return fail(MHPC_ERR_INVALID, "null argument");
  if (n_sets < 1 || n_sets > MHPC_MAX_OPTION_SETS)
    return fail(MHPC_ERR_INVALID, "n_sets must be 1..MHPC_MAX_OPTION_SETS");
  for (int i = 0; i < n_sets; ++i) PLANCHK(check_option, &sets[i], &h->opt.alpha);
  const int B = h->sp.B;
  std::vector<const mhpc_hsddp_option*> want(B);
  for (int b = 0; b < B; ++b) {
    const int i = set_of ? set_of[b] : b % n_sets;
    if (i < 0 || i >= n_sets) return fail(MHPC_ERR_INVALID, "set index out of range");
    want[b] = &sets[i];
  }
  OptTable nt = h->otab;
  std::vector<int> changed;
  PLANCHK(plan_options, nt, want, changed);
  if (changed.empty()) return MHPC_OK;
  std::vector<int> ent(2 * changed.size());
  for (size_t i = 0; i < changed.size(); ++i) {
    ent[2 * i] = changed[i];
    ent[2 * i + 1] = nt.of[changed[i]];
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  DevTemp<int> ti(h->main.s1);
  const int* dent = ti.in(std::move(ent));
  if (ti.e != hipSuccess) return dev_fail("mhpc_set_option_sets", ti.e);
  // ---- nothing of the handle or the device has changed up to here ----
  std::swap(h->otab, nt);
  int rc = upload_options(h);
  if (rc) {  // the old table back, host and device (as far as the device still answers)
    keep_error([&] {
      std::swap(h->otab, nt);
      (void)upload_options(h);
    });
    return rc;
  }
  hipError_t e = launch_set_options(h->d, h->own.oid.get(), (int)changed.size(), dent, 1, h->main.s1);
  if (e == hipSuccess) e = hipStreamSynchronize(h->main.s1);
  if (e != hipSuccess) return dev_fail("mhpc_set_option_sets", e);
  // a problem that now has AL iterations while its SRB nominal is open (Ledger::budget_raised)
  for (int b : changed)
    if (!no_al_iteration(h->otab.rec[h->otab.of[b]]) &&
        h->led.budget_raised(b, !h->need_full && !h->solved && h->initialized))
      h->need_full = true;
  return MHPC_OK;
}
int api_set_options(Handle* h, const mhpc_hsddp_option* o) {
  return api_set_option_sets(h, 1, o, nullptr);
}
int api_get_problem_options(Handle* h, int b, mhpc_hsddp_option* o) {
  if (!h || !o) return fail(MHPC_ERR_INVALID, "null argument");
  if (b < 0 || b >= h->sp.B) return fail(MHPC_ERR_INVALID, "problem out of range");
  *o = h->otab.rec[h->otab.of[b]];
  return MHPC_OK;
}
int api_get_options(Handle* h, mhpc_hsddp_option* o) { return api_get_problem_options(h, 0, o); }
int api_num_option_sets(Handle* h, int* n) {
  if (!h || !n) return fail(MHPC_ERR_INVALID, "null argument");
  *n = h->otab.in_use();
  return MHPC_OK;
}

int api_create(const mhpc_problem_desc* desc, const mhpc_hsddp_option* opt, int batch,
                           int device, Handle** out) {
  if (!out || !opt) return fail(MHPC_ERR_INVALID, "null argument");
  *out = nullptr;
  PLANCHK(check_desc, desc);
  if (batch < 1) return fail(MHPC_ERR_INVALID, "batch must be >= 1");
  PLANCHK(check_option, opt, nullptr);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MHPC_ERR_INVALID, "no such device");
  HIPCHK(hipSetDevice(device));

  Handle* h = new Handle();
  h->desc = norm_desc(*desc);
  h->opt = *opt;
  h->device = device;
  SolveParams& sp = h->sp;
  memset(&sp, 0, sizeof sp);
  sp.B = batch;
  // launch shapes follow this handle's device (one process may hold handles on several)
  if (hipDeviceGetAttribute(&sp.ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      sp.ncu < 1)
    sp.ncu = 256;
  // line-search grid exactly as MultiPhaseDDP::forward_iteration generates it (:130-151)
  const int nc = option_grid(opt->alpha, MAXC, sp.eps);  // (check_option: at most MAXC trials)
  sp.n_cand = nc;
  sp.ro_store = ro_store_default();
  sp.nslot = nc + 1;
  sp.eps9 = pow(0.1, 9);
  sp.min_n_al = sp.min_max_ddp = 0;  // (outside a solve's scope: every kernel reads the records)
  sp.al_uniform = -1;
  // one option set: the record given here, every problem's (upload_options below fills k_init's copy)
  h->otab.rec.assign(1, norm_option(*opt));
  h->otab.use.assign(1, batch);
  h->otab.of.assign(batch, 0);
  {  // the reference's weights and constraint parameters until mhpc_set_* replaces them
    mhpc_cost_weights w;
    mhpc_constraint_params c;
    mhpc_default_cost_weights(&w);
    mhpc_default_constraint_params(&c);
    CostParams cw;
    put_weights(cw, w);
    put_constraints(cw, c);
    h->psets.assign(1, cw);
    h->pset_of.assign(batch, 0);
  }
  h->pl.assign(batch, ProbLayout{h->desc, 0, 0});
  h->led = Ledger(batch);
  h->cmode.assign(batch, desc->mode_seq[0]);

  DevBufs& d = h->d;
  memset(&d, 0, sizeof d);
  const size_t B = batch;
  Handle::Arrays& a = h->own;
  hipError_t e = hipSuccess;
  auto alloc = [&](auto& arr, size_t n) {
    if (e == hipSuccess) e = arr.alloc(n);
  };
  alloc(a.px, B * MAXP * 196);
  alloc(a.x0, B * 14);
  alloc(a.st, B);
  alloc(a.carry, B);
  alloc(h->dcnt, MAXL * NCNT);
  alloc(a.grp, MAXL);
  alloc(a.gidx, B);
  alloc(a.lid, B);
  alloc(h->dsplit, B);
  alloc(a.opt, MAXO);
  alloc(a.oid, B);
  set_views(h);
  if (e == hipSuccess) e = h->main.create(false);
  if (e == hipSuccess) e = h->ev0.create(EV_TIMING);
  if (e == hipSuccess) e = h->ev1.create(EV_TIMING);
  // zero x0 on the handle's own (non-blocking) stream: a null-stream memset would not be
  // ordered before mhpc_set_x0's copy on this stream
  if (e == hipSuccess) e = hipMemsetAsync(d.x0, 0, B * 14 * sizeof(real), h->main.s1);
  if (e == hipSuccess) e = hipMemsetAsync(a.opt.get(), 0, MAXO * sizeof(OptRec), h->main.s1);
  if (e == hipSuccess) e = hipMemsetAsync(a.oid.get(), 0, B * sizeof(int), h->main.s1);  // slot 0
  // every problem starts with the descriptor's command
  h->cmd.resize(2 * B);
  for (size_t b = 0; b < B; ++b) {
    h->cmd[2 * b] = desc->vel_cmd;
    h->cmd[2 * b + 1] = desc->height_cmd;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->main.s1);
  int rc2 = e == hipSuccess ? MHPC_OK : fail(MHPC_ERR_DEVICE, std::string("allocation failed: ") + hipGetErrorString(e));
  if (!rc2) rc2 = upload_options(h);
  if (!rc2) {  // one group; allocates the packed arrays
    GroupPlan plan;
    rc2 = plan_groups(h->pl, h->pset_of, plan, nullptr);  // (one layout, one set: never refused)
    if (!rc2) rc2 = commit_groups(h, std::move(plan), false);
  }
  if (!rc2) {  // the command array (after the packed arrays: their placement stays as it was)
    const std::vector<Cmd> hcmd(B, Cmd{(real)desc->vel_cmd, (real)desc->height_cmd});
    e = a.cmd.alloc(B);
    set_views(h);
    if (e == hipSuccess)
      e = hipMemcpyAsync(a.cmd.get(), hcmd.data(), B * sizeof(Cmd), hipMemcpyHostToDevice, h->main.s1);
    if (e == hipSuccess) e = hipStreamSynchronize(h->main.s1);
    if (e != hipSuccess)
      rc2 = fail(MHPC_ERR_DEVICE, std::string("allocation failed: ") + hipGetErrorString(e));
  }
  if (rc2) {
    api_destroy(h);
    return rc2;
  }
  *out = h;
  return MHPC_OK;
}

// The way back from device rows of 14 (pack_rows, mhpc_plan.h) for rows of one width.
static void unpad_rows(const real* src, size_t rows, int r, double* dst) {
  for (size_t t = 0; t < rows; ++t)
    for (int i = 0; i < r; ++i) dst[t * r + i] = src[t * 14 + i];
}

int api_set_x0(Handle* h, const double* x0) {
  if (!h || !x0) return fail(MHPC_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  const std::vector<real> pad = pack_rows<real>(h->plan, h->sp.B, 1, x0, 0);
  HIPCHK(hipMemcpyAsync(h->d.x0, pad.data(), pad.size() * sizeof(real), hipMemcpyHostToDevice,
                        h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  h->x0_set = true;
  h->x0_changed = true;  // references follow x0 only through initialize / update_problem
  return MHPC_OK;
}

static int mark(Handle* h, int kind, hipStream_t s) {
  if (!h->profile) return MHPC_OK;
  Event e;  // (appended only once recorded: a failure leaves the pool as it was)
  HIPCHK(e.create(EV_TIMING));
  HIPCHK(hipEventRecord(e, s));
  h->evpool.push_back(std::move(e));
  h->evkind.push_back(kind);
  return MHPC_OK;
}
// one launch on stream s, bracketed by profiling events on the same stream
#define LAUNCH_ON(h, kind, s, expr)    \
  do {                                 \
    int rc_ = mark(h, kind, s);        \
    if (rc_) return rc_;               \
    HIPCHK(expr);                      \
    rc_ = mark(h, -1, s);              \
    if (rc_) return rc_;               \
  } while (0)
#define LAUNCH(h, kind, expr) LAUNCH_ON(h, kind, h->main.s1, expr)

static int collect_profile(Handle* h) {
  for (size_t i = 0; i + 1 < h->evpool.size(); i += 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->evpool[i], h->evpool[i + 1]));
    h->kms[h->evkind[i]] += ms;
    h->klaunch[h->evkind[i]] += 1;
  }
  h->evpool.clear();
  h->evkind.clear();
  return MHPC_OK;
}

// Device -> host copy ordered on the handle's stream.
static int d2h(Handle* h, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}
#define D2H(dst, src, bytes)                \
  do {                                      \
    int rc_ = d2h(h, (dst), (src), (bytes)); \
    if (rc_) return rc_;                    \
  } while (0)

// initialization(): memory_reset + build_problem (refs) + warmstart, all on the device.
static int initialize_async(Handle* h) {
  // build_problem binds phase p to buffer p and starts the gait at each problem's first mode
  bool rotated = false;
  for (const ProbLayout& q : h->pl) rotated = rotated || q.rot_wb != 0 || q.rot_fb != 0;
  if (rotated) {
    std::vector<ProbLayout> npl = h->pl;
    for (ProbLayout& q : npl) q.rot_wb = q.rot_fb = 0;
    GroupPlan plan;
    PLANCHK(plan_groups, npl, h->pset_of, plan);
    if (int rc = commit_groups(h, std::move(plan), false, &npl)) return rc;
  }
  for (int b = 0; b < h->sp.B; ++b) h->cmode[b] = h->pl[b].desc.mode_seq[0];
  const SolveParams& sp = h->sp;
  DevBufs& d = h->d;
  // memory_reset (K / du / G, trajectory tails) on the second stream beside k_init, which
  // touches none of it; the first solve op waits for both
  HIPCHK(hipEventRecord(h->main.fork, h->main.s1));
  HIPCHK(hipStreamWaitEvent(h->main.s2, h->main.fork, 0));
  HIPCHK(launch_reset_arrays(sp, d, h->main.s2));
  HIPCHK(hipEventRecord(h->main.join, h->main.s2));
  LAUNCH(h, K_INIT, launch_init(sp, d, h->main.s1));
  // (k_init wrote the AL / ReB initial values of problem 0's set for every problem)
  if (own_init_values(h)) {  // its time and bytes (four MAXP-long arrays a problem) count as k_init's
    LAUNCH(h, K_INIT, launch_init_params(sp, d, 1, h->main.s1));
    h->kbytes[K_INIT] += (double)sp.B * 4 * MAXP * kB;
  }
  HIPCHK(hipStreamWaitEvent(h->main.s1, h->main.join, 0));
  for (int g = 0; g < sp.ngrp; ++g) h->kbytes[K_INIT] += h->plan.bym[g].init * (sp.go[g + 1] - sp.go[g]);
  // the buffer store is zeroed lazily (first update_problem), so a plain initialize + solve
  // pays nothing for it
  h->store_valid = false;
  h->need_full = false;
  h->led.initialized([&](int b) { return no_al_iteration(h->otab.rec[h->otab.of[b]]); });
  return MHPC_OK;
}

// ---- call order ---------------------------------------------------------------------------------
// New x0, commands and constraint parameters reach the problems' references and AL / ReB state only
// through mhpc_initialize / mhpc_update_problem(s): each setter raises its flag on an initialised
// handle, those two call mark_current, and the entry points in between refuse with their own
// message for the flags they look at.
static void mark_current(Handle* h) {
  h->x0_changed = h->params_changed = h->sets_changed = false;
  h->led.all_current();
  h->solved = false;
}
// commands or constraint parameters pending (sets_changed is only ever raised with params_changed)
static bool pending(const Handle* h) { return h->led.cmd_pending() || h->params_changed; }
static const char* const kCmdPending =
    "commands changed: call mhpc_initialize or mhpc_update_problem first";
static const char* const kParamsPending =
    "constraint parameters changed: call mhpc_initialize or mhpc_update_problem first";

int api_initialize(Handle* h) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (!h->x0_set) return fail(MHPC_ERR_STATE, "mhpc_set_x0 must precede mhpc_initialize");
  HIPCHK(hipSetDevice(h->device));
  int rc = initialize_async(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->main.s1));
  rc = collect_profile(h);
  if (rc) return rc;
  h->initialized = true;
  mark_current(h);
  return MHPC_OK;
}

// MultiPhaseDDP::solve (MultiPhaseDDP.cpp:154-289) as a fixed launch schedule; every kernel
// skips the problems whose device state machine has left the corresponding loop.
// With bws_split the partials of an iteration run on the second stream beside the SRB half
// of the backward sweep (which reads no partials record); the WB half waits for them.
//
// Sub-batches (MHPC_VARIANT_SUBBATCH): the same schedule runs once per contiguous block of
// problems, each block on its own stream pair.  Problems are independent and every array is
// problem-major, so a block is a pointer offset and its problems compute exactly what they
// compute in one launch over the whole batch (every launch shape is bitwise the same
// arithmetic, tests/test_gpu_variants.py).  Block s+1 starts one launch behind block s:
// the line search (two thirds of the SIMDs busy at batch 1024, one wave per SIMD) then
// shares the chip with the other block's sweep / partials instead of leaving SIMDs idle.
// (the ops themselves: solve_ops, mhpc_plan.h)
struct SolveBlock {
  SolveParams sp;
  DevBufs d;
  const StreamSet* q = nullptr;  // what it runs on: the handle's main set, or a sub-batch's
  // OP_FULL with fresh problems in the batch (Ledger::fresh): the block's problems split into
  // the rolled-out ones (spf) and the fresh ones (spc, k_cost), both over Handle::dsplit
  bool mixed = false;
  SolveParams spf, spc;
};
// What one run of the solve schedule (solve_async) or of the batch's init kernels covers: the whole
// batch (mhpc_solve) or a list of problems (mhpc_tick_problems, mhpc_reset_problems), built by
// make_scope alone.  sp is a copy of the handle's and d the handle's arrays; the launch variants and
// ro_store follow the scope's problem count through this copy, never through Handle::sp.
struct Scope {
  SolveParams sp;
  DevBufs d;
  int n = 0;           // problems of the scope
  ScopeCaps caps;      // the largest iteration caps among them (scope_caps, mhpc_plan.h)
  bool full = false;   // the first op is the real rollout (a rotated nominal, a new x0)
  // ... with fresh problems in the scope (Ledger::fresh): that op splits into the rolled-out
  // problems and the fresh ones (k_cost) over ss->split (mhpc_plan.h, solve_scope)
  bool mixed = false;
  const SolveScope* ss = nullptr;
};
// The block's two halves for a mixed OP_FULL (scope_split over the block's positions; dsplit: the
// rolled-out problems first, then the fresh ones, each in the scope's order).
static void split_block(SolveBlock& k, const SolveScope& ss) {
  k.mixed = true;
  k.spf = k.spc = k.sp;
  k.spf.ident = k.spc.ident = 0;
  scope_split(ss, k.sp.go, k.spf.go, k.spc.go);
}
// dorder: ss->order on the device -- the scope is that list (ident = 0, go[] counted over it, gidx =
// dorder); null: the whole batch under the handle's own sp and gidx, where ss (may be null) only
// gives the split of a mixed first op.
static Scope make_scope(const Handle* h, const SolveScope* ss, const int* dorder, const ScopeCaps& caps,
                        bool full) {
  Scope sc;
  sc.sp = h->sp;
  sc.d = h->d;
  sc.n = h->sp.B;
  if (dorder) {
    sc.sp.ident = 0;
    std::copy(ss->go, ss->go + MAXL + 1, sc.sp.go);
    sc.d.gidx = dorder;
    sc.n = ss->size();
  }
  sc.caps = caps;
  sc.full = full;
  sc.mixed = full && ss && ss->nnf < sc.n;
  sc.ss = ss;
  return sc;
}

// Problems [b0, b0 + sp.B) of the handle's arrays as the kernels index them (b * per-problem
// stride, with sp.NK the knot stride of the packed arrays): for the layout-free export kernel.
static DevBufs block_bufs(const DevBufs& d, const SolveParams& sp, size_t b0) {
  DevBufs o = d;
  const size_t NK = sp.NK;
  o.traj += b0 * sp.nslot * NK * KS;
  o.refpos += b0 * NK;
  o.K += b0 * NK * 56;
  o.du += b0 * NK * 4;
  o.G += b0 * NK * 14;
  o.par += b0 * NK * PS;
  o.px += b0 * MAXP * 196;
  o.x0 += b0 * 14;
  o.st += b0;
  o.out += b0 * NK * KS;
  o.carry += b0;
  o.cmd += b0;
  o.oid += b0;
  return o;
}

// With bws_split the partials run on the block's second stream beside the SRB half of the
// backward sweep (which reads no partials record); the WB half waits for them.
static int issue_op(Handle* h, const SolveBlock& k, const SolveOp& op) {
  const SolveParams& sp = k.sp;
  const DevBufs& d = k.d;
  const StreamSet& q = *k.q;
  const bool split = bws_split(sp);
#ifdef MHPC_FP32
  auto launch_bws = h->sweep_bits == 32 ? fsweep::launch_bws : MHPC_NS::launch_bws;
#endif
  switch (op.kind) {
    case OP_FULL:
      if (k.mixed) {
        DevBufs ds = d;
        ds.gidx = h->dsplit.get();
        if (launch_problems(k.spf) > 0)
          LAUNCH_ON(h, K_FULL, q.s1, launch_rollout(k.spf, ds, op.al, 0, 1, q.s1));
        if (launch_problems(k.spc) > 0)
          LAUNCH_ON(h, K_FULL, q.s1, launch_cost(k.spc, ds, op.al, q.s1));
        break;
      }
      LAUNCH_ON(h, K_FULL, q.s1, launch_rollout(sp, d, op.al, 0, 1, q.s1));
      break;
    case OP_COST:
      LAUNCH_ON(h, K_FULL, q.s1, launch_cost(sp, d, op.al, q.s1));
      break;
    case OP_PAR:
      if (!split) {
        LAUNCH_ON(h, K_PAR, q.s1, launch_partials(sp, d, op.al, op.ddp, q.s1, q.s3, q.pfork, q.pjoin));
        break;
      }
      HIPCHK(hipEventRecord(q.fork, q.s1));
      HIPCHK(hipStreamWaitEvent(q.s2, q.fork, 0));
      LAUNCH_ON(h, K_PAR, q.s2, launch_partials(sp, d, op.al, op.ddp, q.s2, q.s3, q.pfork, q.pjoin));
      HIPCHK(hipEventRecord(q.join, q.s2));
      break;
    case OP_BWS:
      if (!split) {
        LAUNCH_ON(h, K_BWS, q.s1, launch_bws(sp, d, op.al, op.ddp, 0, q.s1));
        break;
      }
      LAUNCH_ON(h, K_BWS_SRB, q.s1, launch_bws(sp, d, op.al, op.ddp, 1, q.s1));
      HIPCHK(hipStreamWaitEvent(q.s1, q.join, 0));
      LAUNCH_ON(h, K_BWS, q.s1, launch_bws(sp, d, op.al, op.ddp, 2, q.s1));
      break;
    case OP_LS:
      LAUNCH_ON(h, K_LS, q.s1, launch_rollout(sp, d, op.al, op.ddp, 0, q.s1));
      break;
    default:
      LAUNCH_ON(h, K_AL, q.s1, launch_al_end(sp, d, op.al, op.last, q.s1));
  }
  return MHPC_OK;
}

static int sub_batches(const Handle* h, int problems) {
  int n = h->nsub_req;
  if (n == 0) n = 1;  // automatic: one block (DESIGN.md §3 has the measured A/B)
  return std::min(n, problems);
}

static int ensure_sub_streams(Handle* h, int n) {
  HIPCHK(h->evstart.ensure());
  HIPCHK(grow_stream_sets(h->subs, n));
  return MHPC_OK;
}

static int solve_async(Handle* h, Scope& sc) {
  // stored line-search trials for this scope's launch shape (unless set by the caller)
  if (!h->ro_store_req) sc.sp.ro_store = ro_store_auto(sc.sp);
  // what the scope's problems have in common, for the kernels' gates (SolveParams::min_n_al ...)
  sc.sp.min_n_al = sc.caps.min_n_al;
  sc.sp.min_max_ddp = sc.caps.min_max_ddp;
  sc.sp.al_uniform = sc.caps.al_uniform;
  // the schedule runs to the largest iteration caps among the scope's problems
  const std::vector<SolveOp> ops = solve_ops(sc.caps, sc.full);
  const int nops = (int)ops.size();
  const int nsub = sub_batches(h, sc.n);
  int rc;
  // fresh problems in a solve that starts with the real rollout: the split order to the device
  const bool mixed = sc.mixed;
  if (mixed) {
    HIPCHK(hipMemcpyAsync(h->dsplit.get(), sc.ss->split.data(), (size_t)sc.n * sizeof(int),
                          hipMemcpyHostToDevice, h->main.s1));
    HIPCHK(hipStreamSynchronize(h->main.s1));
  }
  if (nsub <= 1) {
    SolveBlock k{sc.sp, sc.d, &h->main};
    if (mixed) split_block(k, *sc.ss);
    for (const SolveOp& op : ops)
      if ((rc = issue_op(h, k, op))) {
        // an issue failure may leave launches queued on the second / third stream (the
        // partials fork onto s3 and join back only at their end): drain both, so no later
        // work on the handle runs unordered with them
        drain({h->main.s3, h->main.s2});
        (void)hipStreamWaitEvent(h->main.s1, h->main.join, 0);
        return rc;
      }
    // a schedule whose last partials have no sweep after them (max_DDP_iter = 0) still
    // joins the second stream back before the solve counts as done
    HIPCHK(hipStreamWaitEvent(h->main.s1, h->main.join, 0));
  } else {
    if ((rc = ensure_sub_streams(h, nsub))) return rc;
    HIPCHK(hipEventRecord(h->evstart, h->main.s1));
    std::vector<SolveBlock> blk(nsub);
    // even partition of the scope's positions: every block non-empty (sub_batches() <= n), sizes
    // differ by <= 1
    const int B = sc.n;
    for (int s = 0; s < nsub; ++s) {
      SolveBlock& k = blk[s];
      const int b0 = (int)((int64_t)s * B / nsub), b1 = (int)((int64_t)(s + 1) * B / nsub);
      // the block's problems: the scope's positions [b0, b1) (each group's range clipped to them);
      // the arrays stay the handle's (gidx holds absolute problem indices)
      k.sp = sc.sp;
      scope_clip(sc.sp.go, sc.sp.ngrp, b0, b1, k.sp.go);
      k.d = sc.d;
      k.q = &h->subs[s];
      if (mixed) split_block(k, *sc.ss);
      HIPCHK(hipStreamWaitEvent(k.q->s1, h->evstart, 0));
    }
    // block s runs `lag` launches behind block s - 1 (its first launch waits on the gate
    // event recorded after launch lag - 1 of the block before; issued in that order)
    int lag = 1;
    if (const char* e = getenv("MHPC_SUB_LAG")) lag = atoi(e);  // tuning only
    lag = std::max(0, std::min(lag, nops - 1));
    // every block's streams are joined back to h->main.s1 even when an issue fails partway,
    // so later work on the handle never races with a block's queued launches
    auto join_all = [&]() -> hipError_t {
      hipError_t e = hipSuccess;
      for (int s = 0; s < nsub; ++s) {
        hipError_t e1 = hipStreamWaitEvent(h->subs[s].s1, h->subs[s].join, 0);
        if (e1 == hipSuccess) e1 = hipEventRecord(h->subs[s].done, h->subs[s].s1);
        if (e1 == hipSuccess) e1 = hipStreamWaitEvent(h->main.s1, h->subs[s].done, 0);
        if (e == hipSuccess) e = e1;
      }
      return e;
    };
    rc = MHPC_OK;
    for (int t = 0; t < nops + (nsub - 1) * lag && !rc; ++t)
      for (int s = 0; s < nsub && !rc; ++s) {
        const int i = t - s * lag;
        if (i < 0 || i >= nops) continue;
        if (s > 0 && i == 0 && lag > 0 &&
            hipStreamWaitEvent(h->subs[s].s1, h->subs[s - 1].gate, 0) != hipSuccess)
          rc = fail(MHPC_ERR_DEVICE, "sub-batch gate wait failed");
        if (!rc) rc = issue_op(h, blk[s], ops[i]);
        if (!rc && s + 1 < nsub && lag > 0 && i == lag - 1 &&
            hipEventRecord(h->subs[s].gate, h->subs[s].s1) != hipSuccess)
          rc = fail(MHPC_ERR_DEVICE, "sub-batch gate record failed");
      }
    const hipError_t ej = join_all();
    if (rc) {  // (as above: the blocks' partials streams drained on an issue failure)
      for (int q = 0; q < nsub; ++q) drain({h->subs[q].s3, h->subs[q].s2});
      return rc;
    }
    HIPCHK(ej);
  }
  // totals of the per-problem counters per group (tiny reduction, NCNT words each)
  HIPCHK(hipMemsetAsync(h->dcnt.get(), 0, (size_t)sc.sp.ngrp * NCNT * sizeof(unsigned long long), h->main.s1));
  HIPCHK(launch_reduce_counters(sc.sp, sc.d, h->dcnt.get(), h->main.s1));
  return MHPC_OK;
}

// The scope of the whole batch: the handle's own sp / gidx; the first op the real rollout after an
// update_problem (need_full), split when a reset left fresh problems (ss: the caller's storage).
static Scope batch_scope(Handle* h, SolveScope& ss) {
  const bool split = h->need_full && h->led.nfresh() > 0;
  if (split) ss = solve_scope(h->plan, h->plan.gidx, h->led.fresh_flags());
  return make_scope(h, split ? &ss : nullptr, nullptr, scope_caps(h->otab, nullptr, 0), h->need_full);
}

// After a scope's solve has drained: its counters (per group, summed over the scope's problems)
// and their byte / flop accounting, the profile.
static int account_solve(Handle* h, const Scope& sc) {
  for (int i = 0; i < NCNT; ++i) {
    h->cnt[i] = 0;
    for (int g = 0; g < sc.sp.ngrp; ++g) h->cnt[i] += h->gcnt[g][i];
  }
  HIPCHK(hipEventElapsedTime(&h->solve_ms, h->ev0, h->ev1));
  const int rc = collect_profile(h);
  if (rc) return rc;
  const unsigned long long* c = h->cnt;
  for (int g = 0; g < sc.sp.ngrp; ++g) {  // per group: its problems' counters x its layout's bytes
    const unsigned long long* cg = h->gcnt[g];
    const ByteModel& m = h->plan.bym[g];
    const SolveParams& sp = sc.sp;
    h->kbytes[K_FULL] += cg[C_FWD] * m.cost;
    // the trials that store their records (RO_STORE_FIRST; the re-rolls of the others, rare,
    // are not counted)
    const double stored = std::min(sp.n_cand, sp.ro_store + 1);
    h->kbytes[K_LS] += cg[C_LS_LAUNCH] * m.roll_read +
                       cg[C_LS_RUN] * (m.roll_write * stored / sp.n_cand + m.roll_term);
    h->kbytes[K_PAR] += cg[C_PAR_RUN] * m.par;
    h->kflops[K_LS] += cg[C_LS_RUN] * m.roll_flops;
  }
  // the SRB half of a split sweep: the SRB knots of every first attempt; the rest (WB knots,
  // impact steps, SRB knots of retries) is the WB half's / the whole sweep's
  const unsigned long long fb1 = c[C_BWS_KNOTS_FB1], fb = c[C_BWS_KNOTS_FB] - fb1;
  h->kbytes[K_BWS_SRB] += fb1 * kBwsFbKnot;
  h->kflops[K_BWS_SRB] += fb1 * kFlopFbKnot;
  h->kbytes[K_BWS] += c[C_BWS_KNOTS_WB] * kBwsWbKnot + fb * kBwsFbKnot + c[C_PX_READS] * kBwsPx;
  h->kflops[K_BWS] += c[C_BWS_KNOTS_WB] * kFlopWbKnot + fb * kFlopFbKnot + c[C_PX_READS] * kFlopPx;
  return MHPC_OK;
}

int api_solve(Handle* h, int32_t* status) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "mhpc_initialize must precede mhpc_solve");
  if (h->solved) return fail(MHPC_ERR_STATE, "solve already ran: call mhpc_initialize or mhpc_update_problem");
  if (h->x0_changed)
    return fail(MHPC_ERR_STATE, "x0 changed: call mhpc_initialize or mhpc_update_problem first");
  if (pending(h)) return fail(MHPC_ERR_STATE, h->params_changed ? kParamsPending : kCmdPending);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventRecord(h->ev0, h->main.s1));
  SolveScope ss;
  Scope sc = batch_scope(h, ss);
  int rc = solve_async(h, sc);
  h->sp.ro_store = sc.sp.ro_store;  // (the batch's own choice stays visible in the handle's sp)
  if (rc) return rc;
  HIPCHK(hipEventRecord(h->ev1, h->main.s1));
  HIPCHK(hipMemcpyAsync(h->gcnt, h->dcnt.get(), (size_t)h->sp.ngrp * NCNT * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  h->solved = true;
  h->need_full = false;
  h->led.solved();
  if ((rc = account_solve(h, sc))) return rc;
  if (status) {
    std::vector<ProbState> st(h->sp.B);
    D2H(st.data(), h->d.st, st.size() * sizeof(ProbState));
    for (int b = 0; b < h->sp.B; ++b) status[b] = st[b].status;
  }
  return MHPC_OK;
}

// Rows [ko, ko + N) of a problem-major [B][NK][per] device array into buf ([B][N][per]):
// one strided copy of just the requested phase (not the whole trajectory buffer).
static int copy_rows(Handle* h, const real* src, int per, int ko, int N, size_t b0, size_t B,
                     std::vector<real>& buf) {
  const size_t NK = h->sp.NK, w = (size_t)N * per * sizeof(real);
  buf.resize(B * N * per);
  HIPCHK(hipMemcpy2DAsync(buf.data(), w, src + (b0 * NK + (size_t)ko) * per,
                          NK * per * sizeof(real), w, B, hipMemcpyDeviceToHost, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}

// Problems [first, first + count) of one phase (count = batch: mhpc_get_phase).  The range's
// phase must have one shape (knots, state size); runs of problems whose phase starts at the
// same knot offset are copied with one strided copy each.
static int get_phase_run(Handle* h, int phase, int n, int N, int ko, size_t b0, size_t B, double* x,
                         double* u, double* y, double* K, double* du, double* Vx) {
  const SolveParams& sp = h->sp;
  std::vector<real> buf;
  int rc;
  if (x || u || y) {
    // export only the requested problems (a caller looping over problems would otherwise
    // export the whole batch per call)
    SolveParams sub = sp;
    sub.B = (int)B;
    HIPCHK(launch_export(sub, block_bufs(h->d, sp, b0), h->main.s1));
    if ((rc = copy_rows(h, h->d.out, KS, ko, N, b0, B, buf))) return rc;
    for (size_t b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k) {
        const real* r = &buf[(b * N + k) * KS];
        for (int i = 0; i < n; ++i)
          if (x) x[(b * N + k) * n + i] = r[i];
        for (int i = 0; i < 4; ++i) {
          if (u) u[(b * N + k) * 4 + i] = r[n + i];
          if (y) y[(b * N + k) * 4 + i] = r[n + 4 + i];
        }
      }
  }
  if (K) {
    if ((rc = copy_rows(h, h->d.K, 56, ko, N, b0, B, buf))) return rc;
    for (size_t b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k)
        for (int i = 0; i < 4 * n; ++i) K[(b * N + k) * 4 * n + i] = buf[(b * N + k) * 56 + i];
  }
  if (du) {
    if ((rc = copy_rows(h, h->d.du, 4, ko, N, b0, B, buf))) return rc;
    for (size_t i = 0; i < B * N * 4; ++i) du[i] = buf[i];
  }
  if (Vx) {
    if ((rc = copy_rows(h, h->d.G, 14, ko, N, b0, B, buf))) return rc;
    for (size_t b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k)
        for (int i = 0; i < n; ++i) Vx[(b * N + k) * n + i] = buf[(b * N + k) * 14 + i];
  }
  return MHPC_OK;
}

// Runs of consecutive problems of [first, first + count) with the same key(b): run(r0, n) for
// each in turn, until one returns non-zero (returned).
template <class Key, class Run>
static int for_runs(int first, int count, Key key, Run run) {
  for (int r0 = first, r1; r0 < first + count; r0 = r1) {
    for (r1 = r0 + 1; r1 < first + count && key(r1) == key(r0); ++r1) {
    }
    if (int rc = run(r0, r1 - r0)) return rc;
  }
  return 0;
}

// Shape check of a phase over a problem range: *n, *N of the phase (one shape for the range)
static int range_phase_shape(const Handle* h, int phase, int first, int count, int* n, int* N) {
  if (first < 0 || count < 1 || first > h->sp.B - count)
    return fail(MHPC_ERR_INVALID, "problem range outside the batch");
  for (int b = first; b < first + count; ++b) {
    const Layout& L = h->plan.lays[h->plan.lid[b]];
    if (phase < 0 || phase >= L.P) return fail(MHPC_ERR_INVALID, "bad phase");
    if (b == first) {
      *n = L.xs[phase];
      *N = L.N[phase];
    } else if (L.xs[phase] != *n || L.N[phase] != *N) {
      return fail(MHPC_ERR_INVALID, "the phase differs in shape across the problem range (per-problem layouts)");
    }
  }
  return MHPC_OK;
}

int api_get_phase(Handle* h, int phase, int first, int count, double* x, double* u, double* y,
                  double* K, double* du, double* Vx) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  int n = 0, N = 0;
  int rc = range_phase_shape(h, phase, first, count, &n, &N);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  auto ko = [&](int b) { return h->plan.lays[h->plan.lid[b]].ko[phase]; };
  return for_runs(first, count, ko, [&](int r0, int nb) {
    const size_t o = (size_t)(r0 - first) * N;
    auto at = [&](double* p, int per) { return p ? p + o * per : nullptr; };
    return get_phase_run(h, phase, n, N, ko(r0), r0, nb, at(x, n), at(u, 4), at(y, 4), at(K, 4 * n),
                         at(du, 4), at(Vx, n));
  });
}

int api_get_scalars(Handle* h, double* J, double* dV_exp, double* viol,
                                double* V_phase, double* dV_phase, int32_t* trace) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  HIPCHK(hipSetDevice(h->device));
  const SolveParams& sp = h->sp;
  std::vector<ProbState> st(sp.B);
  D2H(st.data(), h->d.st, st.size() * sizeof(ProbState));
  for (int b = 0; b < sp.B; ++b) {
    if (J) J[b] = st[b].J;
    if (dV_exp) dV_exp[b] = st[b].dV_exp;
    if (viol) viol[b] = st[b].viol;
    // rows of the most phases any layout has; zero past the problem's own phases
    const int P = h->plan.lays[h->plan.lid[b]].P;
    for (int p = 0; p < sp.pmax; ++p) {
      if (V_phase) V_phase[b * sp.pmax + p] = p < P ? (double)st[b].V[p] : 0.0;
      if (dV_phase) dV_phase[b * sp.pmax + p] = p < P ? (double)st[b].dV[p] : 0.0;
    }
    if (trace) memcpy(&trace[(size_t)b * TRACE], st[b].trace, TRACE * sizeof(int32_t));
  }
  return MHPC_OK;
}

// MHPC_ERR_DEVICE naming the entry point fn and the HIP error
static int dev_fail(const char* fn, hipError_t e) {
  return fail(MHPC_ERR_DEVICE, std::string(fn) + ": " + hipGetErrorString(e));
}
// One launch on the handle's stream between its ev0 / ev1, the outputs of t staged after it,
// and the launch's time to *ms (ms may be null); all of it folded into t.e.
template <class Temp, class Launch>
static void timed_launch(Handle* h, Temp& t, float* ms, Launch launch) {
  if (t.e == hipSuccess) t.e = hipEventRecord(h->ev0, h->main.s1);
  if (t.e == hipSuccess) t.e = launch();
  if (t.e == hipSuccess) t.e = hipEventRecord(h->ev1, h->main.s1);
  t.stage();
  float el = 0;
  if (t.e == hipSuccess) t.e = hipEventElapsedTime(&el, h->ev0, h->ev1);
  if (t.e == hipSuccess && ms) *ms = el;
}

int api_rollout_costs(Handle* h, int n_eps, const double* eps, double* J,
                                  double* viol, float* ms) {
  if (!h || !eps || !J) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  if (n_eps < 1 || n_eps > MHPC_MAX_ROLLOUT_EPS) return fail(MHPC_ERR_INVALID, "n_eps out of range");
  if (h->led.cmd_pending()) return fail(MHPC_ERR_STATE, kCmdPending);
  if (h->sets_changed)
    return fail(MHPC_ERR_STATE,
                "parameter sets changed: call mhpc_initialize or mhpc_update_problem first");
  HIPCHK(hipSetDevice(h->device));
  const size_t n = (size_t)h->sp.B * n_eps;
  DevTemp<real> t(h->main.s1);
  real *deps = t.in(eps, n_eps), *dJ = t.out(J, n), *dv = t.out(viol, n);
  timed_launch(h, t, ms,
               [&] { return launch_eps_rollout(h->sp, h->d, n_eps, deps, dJ, dv, h->main.s1); });
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_rollout_costs", t.e);
  return MHPC_OK;
}

// ---- policy rollouts from states of the caller's choosing (k_policy_rollout) ---------------
// Call-order rules shared by the policy entry points: an initialised handle (mhpc_set_layouts
// un-initialises it) with no commands or constraint parameters pending, as mhpc_rollout_costs;
// a pending x0 does not matter to the rollouts, which never read the handle's x0.
static int policy_ready(const Handle* h) {
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  if (pending(h)) return fail(MHPC_ERR_STATE, h->led.cmd_pending() ? kCmdPending : kParamsPending);
  return MHPC_OK;
}
// Caller rows xs [count][n_s][r] of problems [first, first + count) as the device rows of 14
// (mhpc_set_x0's padding and, for E = real, rounding); MHPC_ERR_INVALID for a non-finite entry
// of what.
template <class E>
static int policy_pack(const Handle* h, int first, int count, int n_s, const double* xs,
                       const char* what, std::vector<E>& out) {
  for (size_t i = 0; i < (size_t)count * n_s * x0_row_of(h->plan); ++i)
    if (!std::isfinite(xs[i])) return fail(MHPC_ERR_INVALID, std::string(what) + " must be finite");
  out = pack_rows<E>(h->plan, count, n_s, xs, first);
  return MHPC_OK;
}
static int min_phases(const Handle* h) {
  int P = MAXP;
  for (const Layout& L : h->plan.lays) P = std::min(P, L.P);
  return P;
}

int api_rollout_policy(Handle* h, int n_samples, const double* xs, int n_phases, double* J,
                       double* viol, double* x_end, float* ms) {
  if (!h || !xs || !J) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = policy_ready(h);
  if (rc) return rc;
  if (n_samples < 1 || n_samples > MHPC_MAX_POLICY_SAMPLES)
    return fail(MHPC_ERR_INVALID, "n_samples out of range");
  if (n_phases < 0 || n_phases > min_phases(h))
    return fail(MHPC_ERR_INVALID, "n_phases out of range");
  const int B = h->sp.B;
  const size_t n = (size_t)B * n_samples;
  std::vector<real> hxs;
  if ((rc = policy_pack(h, 0, B, n_samples, xs, "start states", hxs))) return rc;
  HIPCHK(hipSetDevice(h->device));
  DevTemp<real> t(h->main.s1);
  real *dxs = t.in(std::move(hxs)), *dJ = t.out(J, n), *dv = t.out(viol, n);
  real* dxe = x_end ? t.out(nullptr, n * 14) : nullptr;
  timed_launch(h, t, ms, [&] {
    return launch_policy_rollout(h->sp, h->d, n_samples, 0, B, dxs, nullptr, n_phases, 0, dJ, dv,
                                 dxe, nullptr, h->main.s1);
  });
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_rollout_policy", t.e);
  if (x_end) unpad_rows(t.staged(dxe), n, x0_row_of(h->plan), x_end);
  return MHPC_OK;
}

int api_rollout_policy_phase(Handle* h, int phase, int first, int count, int n_samples,
                             const double* xs, double* x, double* u, double* y) {
  if (!h || !xs) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = policy_ready(h);
  if (rc) return rc;
  if (n_samples < 1 || n_samples > MHPC_MAX_POLICY_SAMPLES)
    return fail(MHPC_ERR_INVALID, "n_samples out of range");
  int nx = 0, N = 0;
  if ((rc = range_phase_shape(h, phase, first, count, &nx, &N))) return rc;
  const size_t S = n_samples, n = (size_t)count * S;
  std::vector<real> hxs;
  if ((rc = policy_pack(h, first, count, n_samples, xs, "start states", hxs))) return rc;
  HIPCHK(hipSetDevice(h->device));
  DevTemp<real> t(h->main.s1);
  real *dxs = t.in(std::move(hxs)), *drec = t.out(nullptr, n * N * PREC_W);
  if (t.e == hipSuccess)
    t.e = launch_policy_rollout(h->sp, h->d, n_samples, first, count, dxs, nullptr, 0, phase, nullptr,
                                nullptr, nullptr, drec, h->main.s1);
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_rollout_policy_phase", t.e);
  // device records [count][N][PREC_W][n_s] (the sample fastest: coalesced stores); the last
  // knot has no u, y and an SRB knot no y: zero rows
  const real* hrec = t.staged(drec);
  const bool wb = nx == 14;
  for (size_t b = 0; b < (size_t)count; ++b)
    for (size_t s = 0; s < S; ++s)
      for (int k = 0; k < N; ++k) {
        const real* rk = &hrec[((b * N + k) * PREC_W) * S + s];
        const size_t o = (b * S + s) * N + k;
        for (int i = 0; i < nx; ++i)
          if (x) x[o * nx + i] = rk[(size_t)i * S];
        for (int i = 0; i < 4; ++i) {
          if (u) u[o * 4 + i] = k < N - 1 ? (double)rk[(size_t)(14 + i) * S] : 0.0;
          if (y) y[o * 4 + i] = (k < N - 1 && wb) ? (double)rk[(size_t)(18 + i) * S] : 0.0;
        }
      }
  return MHPC_OK;
}

// Device-side closed loop: x0[b] <- the end state of one policy rollout of problem b over
// n_phases phases from x0[b] + dx[b]; the kernel reads each x0 row before it writes it.
int api_advance_x0(Handle* h, int n_phases, const double* dx) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  int rc = policy_ready(h);
  if (rc) return rc;
  if (n_phases < 1 || n_phases > min_phases(h))
    return fail(MHPC_ERR_INVALID, "n_phases out of range");
  for (const Layout& L : h->plan.lays)
    if (L.n_wb > 0 && n_phases - 1 >= L.n_wb)
      return fail(MHPC_ERR_INVALID,
                  "phase n_phases-1 is an SRB phase: its end state cannot start a whole-body horizon");
  const int B = h->sp.B;
  std::vector<double> hdx;
  if (dx && (rc = policy_pack(h, 0, B, 1, dx, "dx", hdx))) return rc;
  HIPCHK(hipSetDevice(h->device));
  DevTemp<real> t(h->main.s1);
  const double* ddx = dx ? t.in_double(std::move(hdx)) : nullptr;  // added in double
  if (t.e == hipSuccess)
    t.e = launch_policy_rollout(h->sp, h->d, 1, 0, B, h->d.x0, ddx, n_phases, 0, nullptr, nullptr,
                                h->d.x0, nullptr, h->main.s1);
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_advance_x0", t.e);  // no outputs: the sync
  h->x0_set = true;
  h->x0_changed = true;  // as after mhpc_set_x0
  return MHPC_OK;
}

int api_get_x0(Handle* h, double* x0) {
  if (!h || !x0) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  HIPCHK(hipSetDevice(h->device));
  std::vector<real> buf((size_t)h->sp.B * 14);
  D2H(buf.data(), h->d.x0, buf.size() * sizeof(real));
  unpad_rows(buf.data(), h->sp.B, x0_row_of(h->plan), x0);
  return MHPC_OK;
}

// ---- device-resident I/O: the checks and uploads its entry points share ----------------------
// (control: k_control, k_x0_in, mhpc_control.hip; plan export: k_plan_export, k_results_export,
// mhpc_plan_export.hip; plan import: k_plan_import, mhpc_plan_import.hip; one map for the three,
// mhpc_step_map.h)
namespace sm = mhpc_steps;
static_assert((int)sm::STEPS_CONTROL == MHPC_STEPS_CONTROL && (int)sm::STEPS_ALL == MHPC_STEPS_ALL,
              "mhpc_step_map.h restates the scopes of mhpc_capi.h");

static const Layout& problem_layout(const Handle* h, int b) { return h->plan.lays[h->plan.lid[b]]; }
// steps [n] (null: nothing to check) of problems [n] (null: problem i) against the map the
// kernels run, each on its problem's own layout; `refusal` is the message of a step outside it
static int check_steps(const Handle* h, int n, const int32_t* problems, const int32_t* step,
                       int scope, const char* refusal) {
  for (int i = 0; step && i < n; ++i) {
    const Layout& L = problem_layout(h, problems ? problems[i] : i);
    sm::Knot q;
    if (!sm::knot_of(scope, L.P, L.n_wb, L.N, L.ko, step[i], &q))
      return fail(MHPC_ERR_INVALID, refusal);
  }
  return MHPC_OK;
}
// The list of a plan / results call: problems [n] checked (ProblemList), or null for the whole
// batch in order (n == batch).
static int check_list(const Handle* h, int n, const int32_t* problems) {
  if (!problems) {
    if (n != h->sp.B) return fail(MHPC_ERR_INVALID, "n must be the batch when problems is null");
    return MHPC_OK;
  }
  ProblemList listed;
  PLANCHK(listed.begin, n, h->sp.B, false);
  for (int i = 0; i < n; ++i) PLANCHK(listed.add, problems[i]);
  return MHPC_OK;
}
// A window call, in this order: the list, the window, the scope, every first step.
static int check_window_call(const Handle* h, int n, const int32_t* problems,
                             const int32_t* first_step, int window, int scope,
                             const char* step_refusal) {
  if (int rc = check_list(h, n, problems)) return rc;
  if (window < 1 || window > MHPC_MAX_KNOTS)
    return fail(MHPC_ERR_INVALID, "window must be 1..MHPC_MAX_KNOTS");
  if (!sm::scope_ok(scope))
    return fail(MHPC_ERR_INVALID, "scope must be MHPC_STEPS_CONTROL or MHPC_STEPS_ALL");
  return check_steps(h, n, problems, first_step, scope, step_refusal);
}
// The list and the first steps as temporaries of the call (no array of the handle); null for null.
static void upload_list(DevTemp<int>& t, int n, const int32_t* problems, const int32_t* first_step,
                        const int** dlist, const int** dfirst) {
  *dlist = problems ? t.in(std::vector<int>(problems, problems + n)) : nullptr;
  if (dfirst) *dfirst = first_step ? t.in(std::vector<int>(first_step, first_step + n)) : nullptr;
}

// One array of the caller's, as an entry point's table lists it: null when not given; ld the
// elements between two listed problems' blocks (0: dense) of a window block of `kind`
// (mhpc_step_map.h), kind < 0 for an array that is no window block.
struct CallerArray {
  const void* p;
  int64_t ld;
  int kind;
  const char* name;
};
static bool any_given(const CallerArray* a, int na) {
  for (int k = 0; k < na; ++k)
    if (a[k].p) return true;
  return false;
}
// The table's window blocks as the launchers take them: arrays [by kind].
template <class P>
static void arrays_by_kind(const CallerArray* a, int na, P* arrays) {
  for (int k = 0; k < na; ++k)
    if (a[k].kind >= 0) arrays[a[k].kind] = const_cast<P>(a[k].p);
}
// The strides the kernel gets, ld [by kind]: the dense block, or a given array's own ld, which is
// at least that.
static int check_lds(const CallerArray* a, int na, int r, int window, long* ld) {
  for (int k = 0; k < na; ++k) {
    if (a[k].kind < 0) continue;
    const long dense = sm::block(a[k].kind, r, window);
    ld[a[k].kind] = dense;
    if (!a[k].p || a[k].ld == 0) continue;
    if (a[k].ld < dense)
      return fail(MHPC_ERR_INVALID, std::string("ld_") + a[k].name + " below the dense block");
    ld[a[k].kind] = (long)a[k].ld;
  }
  return MHPC_OK;
}
// A caller's device array: device memory of the handle's device, as hipPointerGetAttributes
// reports it (a host pointer, registered or not, or managed memory is refused).
static int check_device_ptr(const Handle* h, const void* p, const char* what) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unknown pointer is an error of the query, not of the device)
    return fail(MHPC_ERR_INVALID, std::string(what) + " is not device memory");
  }
  if (at.type != hipMemoryTypeDevice || at.device != h->device)
    return fail(MHPC_ERR_INVALID, std::string(what) + " is not device memory of the handle's device");
  return MHPC_OK;
}
static int check_device_ptrs(const Handle* h, const CallerArray* a, int na) {
  for (int k = 0; k < na; ++k)
    if (int rc = a[k].p ? check_device_ptr(h, a[k].p, a[k].name) : MHPC_OK) return rc;
  return MHPC_OK;
}
static int check_dev_dtype(int dtype) {
  if (dtype != MHPC_DEV_F64 && dtype != MHPC_DEV_F32)
    return fail(MHPC_ERR_INVALID, "dtype must be MHPC_DEV_F64 or MHPC_DEV_F32");
  return MHPC_OK;
}
// The handle's stream behind everything queued on the caller's stream at this call: an event
// recorded there (created at the first such call), no host-side wait.
static int wait_for_caller(Handle* h, void* stream) {
  HIPCHK(h->evctl.ensure());
  HIPCHK(hipEventRecord(h->evctl, (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(h->main.s1, h->evctl, 0));
  return MHPC_OK;
}
// The steps to the handle's device array [B] (allocated at the first call with steps, after every
// other array of the handle: their placement stays as it was); *dstep null for null steps.
static int upload_steps(Handle* h, const int32_t* step, const int** dstep) {
  *dstep = nullptr;
  if (!step) return MHPC_OK;
  if (!h->dstep.get()) HIPCHK(h->dstep.alloc(h->sp.B));
  h->hstep.assign(step, step + h->sp.B);  // (the copy may outlive a call that fails after it)
  HIPCHK(hipMemcpyAsync(h->dstep.get(), h->hstep.data(), (size_t)h->sp.B * sizeof(int),
                        hipMemcpyHostToDevice, h->main.s1));
  *dstep = h->dstep.get();
  return MHPC_OK;
}

// ---- device-resident control I/O (k_control, k_x0_in: mhpc_control.hip) ---------------------
// Every check of the control entry points that needs no device: the call order (policy_ready),
// every problem's step.
static int control_ready(const Handle* h, const int32_t* step) {
  if (int rc = policy_ready(h)) return rc;
  return check_steps(h, h->sp.B, nullptr, step, sm::STEPS_CONTROL,
                     "control step outside 0..mhpc_num_control_steps - 1");
}

int api_num_plan_steps(Handle* h, int b, int scope, int* n) {
  if (!h || !n) return fail(MHPC_ERR_INVALID, "null argument");
  if (b < 0 || b >= h->sp.B) return fail(MHPC_ERR_INVALID, "problem out of range");
  if (!sm::scope_ok(scope))
    return fail(MHPC_ERR_INVALID, "scope must be MHPC_STEPS_CONTROL or MHPC_STEPS_ALL");
  const Layout& L = problem_layout(h, b);
  *n = sm::n_steps(scope, L.P, L.n_wb, L.N);
  return MHPC_OK;
}
int api_num_control_steps(Handle* h, int b, int* n) {
  return api_num_plan_steps(h, b, sm::STEPS_CONTROL, n);
}

// Host flavour: the arrays staged through device temporaries of double, the same kernel.
int api_control(Handle* h, const int32_t* step, const double* x, double* u, double* x_nom,
                double* u_nom, double* K) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (u && !x) return fail(MHPC_ERR_INVALID, "null x");
  int rc = control_ready(h, step);
  if (rc) return rc;
  const size_t B = h->sp.B, r = x0_row_of(h->plan);
  for (size_t i = 0; x && i < B * r; ++i)
    if (!std::isfinite(x[i])) return fail(MHPC_ERR_INVALID, "x must be finite");
  HIPCHK(hipSetDevice(h->device));
  const int* dstep;
  if ((rc = upload_steps(h, step, &dstep))) return rc;
  DevTemp<double> t(h->main.s1);
  const double* dx = u ? t.in(x, B * r) : nullptr;
  double* du = u ? t.out(u, B * 4) : nullptr;
  double* dxn = x_nom ? t.out(x_nom, B * r) : nullptr;
  double* dun = u_nom ? t.out(u_nom, B * 4) : nullptr;
  double* dK = K ? t.out(K, B * 4 * r) : nullptr;
  if (t.e == hipSuccess)
    t.e = launch_control(h->sp, h->d, dstep, dx, (long)r, du, 4, dxn, dun, dK, (int)r, MHPC_DEV_F64,
                         h->main.s1);
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_control", t.e);
  return MHPC_OK;
}

int api_control_device(Handle* h, const int32_t* step, const void* x, int64_t ldx, void* u,
                       int64_t ldu, void* x_nom, void* u_nom, void* K, int dtype, void* stream) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (u && !x) return fail(MHPC_ERR_INVALID, "null x");
  int rc = control_ready(h, step);
  if (rc) return rc;
  if ((rc = check_dev_dtype(dtype))) return rc;
  const int r = x0_row_of(h->plan);
  if (u && (ldx < r || ldu < 4)) return fail(MHPC_ERR_INVALID, "ldx < r or ldu < 4");
  HIPCHK(hipSetDevice(h->device));
  const CallerArray tab[] = {{u ? x : nullptr, 0, -1, "x"}, {u, 0, -1, "u"},
                             {x_nom, 0, -1, "x_nom"},       {u_nom, 0, -1, "u_nom"},
                             {K, 0, -1, "K"}};
  if ((rc = check_device_ptrs(h, tab, 5))) return rc;
  const int* dstep;
  if ((rc = upload_steps(h, step, &dstep))) return rc;
  if ((rc = wait_for_caller(h, stream))) return rc;
  HIPCHK(launch_control(h->sp, h->d, dstep, u ? x : nullptr, (long)ldx, u, (long)ldu, x_nom, u_nom,
                        K, r, dtype, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}

int api_set_x0_device(Handle* h, const void* x0, int64_t ld, int dtype, void* stream) {
  if (!h || !x0) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = check_dev_dtype(dtype);
  if (rc) return rc;
  if (ld < x0_row_of(h->plan)) return fail(MHPC_ERR_INVALID, "ld < r");
  HIPCHK(hipSetDevice(h->device));
  if ((rc = check_device_ptr(h, x0, "x0"))) return rc;
  if ((rc = wait_for_caller(h, stream))) return rc;
  HIPCHK(launch_x0_in(h->sp, h->d, x0, (long)ld, dtype, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  h->x0_set = true;
  h->x0_changed = true;  // as after mhpc_set_x0
  return MHPC_OK;
}

// ---- device-resident plan export (k_plan_export, k_results_export: mhpc_plan_export.hip) ----
int api_export_plan_device(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                           int window, const mhpc_plan_out* out, int dtype, void* stream,
                           float* ms) {
  if (!h || !out) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = policy_ready(h);
  if (rc) return rc;
  if ((rc = check_dev_dtype(dtype))) return rc;
  if ((rc = check_window_call(h, n, problems, first_step, window, sm::STEPS_CONTROL,
                              "first step outside 0..mhpc_num_control_steps - 1")))
    return rc;
  const int r = x0_row_of(h->plan);
  const CallerArray tab[sm::NOUT + 1] = {{out->x_nom, out->ld_x_nom, sm::X_NOM, "x_nom"},
                                         {out->u_nom, out->ld_u_nom, sm::U_NOM, "u_nom"},
                                         {out->K, out->ld_K, sm::GAIN, "K"},
                                         {out->du, out->ld_du, sm::DU, "du"},
                                         {out->Vx, out->ld_Vx, sm::VX, "Vx"},
                                         {out->y, out->ld_y, sm::Y, "y"},
                                         {out->mode, out->ld_mode, sm::MODE, "mode"},
                                         {out->valid, 0, -1, "valid"}};
  long ld[sm::NOUT];
  if ((rc = check_lds(tab, sm::NOUT + 1, r, window, ld))) return rc;
  if (!any_given(tab, sm::NOUT + 1)) return fail(MHPC_ERR_INVALID, "no array wanted");
  HIPCHK(hipSetDevice(h->device));
  if ((rc = check_device_ptrs(h, tab, sm::NOUT + 1))) return rc;
  void* arrays[sm::NOUT];
  arrays_by_kind(tab, sm::NOUT + 1, arrays);
  DevTemp<int> t(h->main.s1);
  const int *dlist, *dfirst;
  upload_list(t, n, problems, first_step, &dlist, &dfirst);
  if (t.e != hipSuccess) return dev_fail("mhpc_export_plan_device", t.e);
  if ((rc = wait_for_caller(h, stream))) return rc;
  timed_launch(h, t, ms, [&] {
    return launch_plan_export(h->sp, h->d, n, dlist, dfirst, window, r, arrays, ld, out->valid,
                              dtype, h->main.s1);
  });
  if (t.e != hipSuccess) return dev_fail("mhpc_export_plan_device", t.e);
  return MHPC_OK;
}

int api_export_results_device(Handle* h, int n, const int32_t* problems,
                              const mhpc_results_out* out, int dtype, void* stream) {
  if (!h || !out) return fail(MHPC_ERR_INVALID, "null argument");
  int rc = policy_ready(h);
  if (rc) return rc;
  if ((rc = check_dev_dtype(dtype))) return rc;
  if ((rc = check_list(h, n, problems))) return rc;
  const CallerArray tab[6] = {  // the launcher's arrays [5], then status
      {out->J, 0, -1, "J"},       {out->dV_exp, 0, -1, "dV_exp"},
      {out->viol, 0, -1, "viol"}, {out->V_phase, 0, -1, "V_phase"},
      {out->dV_phase, 0, -1, "dV_phase"}, {out->status, 0, -1, "status"}};
  if (!any_given(tab, 6)) return fail(MHPC_ERR_INVALID, "no array wanted");
  HIPCHK(hipSetDevice(h->device));
  if ((rc = check_device_ptrs(h, tab, 6))) return rc;
  void* arrays[5];
  for (int k = 0; k < 5; ++k) arrays[k] = const_cast<void*>(tab[k].p);
  DevTemp<int> t(h->main.s1);
  const int* dlist;
  upload_list(t, n, problems, nullptr, &dlist, nullptr);
  if (t.e != hipSuccess) return dev_fail("mhpc_export_results_device", t.e);
  if ((rc = wait_for_caller(h, stream))) return rc;
  t.e = launch_results_export(h->d, n, dlist, h->sp.pmax, arrays, out->status, dtype, h->main.s1);
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_export_results_device", t.e);  // the sync
  return MHPC_OK;
}

// ---- device-resident plan import (k_plan_import: mhpc_plan_import.hip) -----------------------
// Every check of an import that needs no device: the call order (policy_ready), the window call,
// which arrays of tab [NIN] are given and their leading dimensions; arrays [NIN] and ld [NIN], by
// kind: what the kernel gets.
static int import_ready(const Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                        int window, int scope, const CallerArray* tab, const void** arrays,
                        long* ld) {
  int rc = policy_ready(h);
  if (rc) return rc;
  if ((rc = check_window_call(h, n, problems, first_step, window, scope,
                              "first step outside 0..mhpc_num_plan_steps - 1")))
    return rc;
  arrays_by_kind(tab, sm::NIN, arrays);
  if (!arrays[sm::U_NOM]) return fail(MHPC_ERR_INVALID, "null u_nom");
  if (arrays[sm::GAIN] && !arrays[sm::X_NOM])
    return fail(MHPC_ERR_INVALID, "K without x_nom: the gains act on x - x_nom");
  if (arrays[sm::X_NOM] && !arrays[sm::GAIN]) return fail(MHPC_ERR_INVALID, "x_nom without K");
  return check_lds(tab, sm::NIN, x0_row_of(h->plan), window, ld);
}
// The ledger's side of a finished import (Ledger::guessed): the listed problems' next first sweep
// is the real rollout.
static void import_done(Handle* h, int n, const int32_t* problems) {
  for (int i = 0; i < n; ++i)
    if (h->led.guessed(problems ? problems[i] : i, !h->need_full && !h->solved && h->initialized))
      h->need_full = true;
}

int api_import_plan_device(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                           int window, int scope, const mhpc_plan_in* in, int dtype, void* stream,
                           float* ms) {
  if (!h || !in) return fail(MHPC_ERR_INVALID, "null argument");
  const CallerArray tab[sm::NIN] = {{in->x_nom, in->ld_x_nom, sm::X_NOM, "x_nom"},
                                    {in->u_nom, in->ld_u_nom, sm::U_NOM, "u_nom"},
                                    {in->K, in->ld_K, sm::GAIN, "K"}};
  const void* arrays[sm::NIN];
  long ld[sm::NIN];
  int rc = import_ready(h, n, problems, first_step, window, scope, tab, arrays, ld);
  if (rc) return rc;
  if ((rc = check_dev_dtype(dtype))) return rc;
  HIPCHK(hipSetDevice(h->device));
  if ((rc = check_device_ptrs(h, tab, sm::NIN))) return rc;
  DevTemp<int> t(h->main.s1);
  const int *dlist, *dfirst;
  upload_list(t, n, problems, first_step, &dlist, &dfirst);
  if (t.e != hipSuccess) return dev_fail("mhpc_import_plan_device", t.e);
  if ((rc = wait_for_caller(h, stream))) return rc;
  // ---- nothing of the handle or the device has changed up to here ----
  timed_launch(h, t, ms, [&] {
    return launch_plan_import(h->sp, h->d, n, dlist, dfirst, window, scope, x0_row_of(h->plan),
                              arrays, ld, dtype, h->main.s1);
  });
  if (t.e != hipSuccess) return dev_fail("mhpc_import_plan_device", t.e);
  import_done(h, n, problems);
  return MHPC_OK;
}

// Host flavour: dense double arrays staged through device temporaries of double, the same kernel.
int api_import_plan(Handle* h, int n, const int32_t* problems, const int32_t* first_step,
                    int window, int scope, const double* u_nom, const double* K,
                    const double* x_nom) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  const CallerArray tab[sm::NIN] = {
      {x_nom, 0, sm::X_NOM, "x_nom"}, {u_nom, 0, sm::U_NOM, "u_nom"}, {K, 0, sm::GAIN, "K"}};
  const void* host[sm::NIN];
  long ld[sm::NIN];
  int rc = import_ready(h, n, problems, first_step, window, scope, tab, host, ld);
  if (rc) return rc;
  // every entry the kernel would read is finite: every column of the valid rows that the map
  // does not skip for the row's knot
  const int r = x0_row_of(h->plan);
  const sm::Dims D = {h->sp.NK, h->sp.nslot};
  for (int i = 0; i < n; ++i) {
    const Layout& L = problem_layout(h, problems ? problems[i] : i);
    const int first = first_step ? first_step[i] : 0;
    const int nvalid = sm::valid(sm::n_steps(scope, L.P, L.n_wb, L.N), first, window);
    for (int w = 0; w < nvalid; ++w) {
      sm::Knot q;
      sm::knot_of(scope, L.P, L.n_wb, L.N, L.ko, first + w, &q);
      for (int k = 0; k < sm::NIN; ++k) {
        if (!host[k]) continue;
        const int nc = sm::cols(k, r);
        const double* row = (const double*)host[k] + (size_t)i * ld[k] + (size_t)w * nc;
        size_t off;
        for (int c = 0; c < nc; ++c)
          if (sm::knot_elem(k, r, D, 0, 0, q, c, &off) && !std::isfinite(row[c]))
            return fail(MHPC_ERR_INVALID, "u_nom, K and x_nom must be finite");
      }
    }
  }
  HIPCHK(hipSetDevice(h->device));
  DevTemp<int> t(h->main.s1);
  DevTemp<double> td(h->main.s1);
  const int *dlist, *dfirst;
  upload_list(t, n, problems, first_step, &dlist, &dfirst);
  const void* dev[sm::NIN];
  for (int k = 0; k < sm::NIN; ++k)
    dev[k] = host[k] ? td.in((const double*)host[k], (size_t)n * ld[k]) : nullptr;
  if (t.e != hipSuccess) return dev_fail("mhpc_import_plan", t.e);
  if (td.e != hipSuccess) return dev_fail("mhpc_import_plan", td.e);
  // ---- nothing of the handle or the device has changed up to here ----
  timed_launch(h, t, nullptr, [&] {
    return launch_plan_import(h->sp, h->d, n, dlist, dfirst, window, scope, r, dev, ld,
                              MHPC_DEV_F64, h->main.s1);
  });
  if (t.e != hipSuccess) return dev_fail("mhpc_import_plan", t.e);
  import_done(h, n, problems);
  return MHPC_OK;
}

int api_get_cost_gradients(Handle* h, int phase, int first, int count, double* lx, double* Phix) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  int n = 0, N = 0;
  int rc = range_phase_shape(h, phase, first, count, &n, &N);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  DevTemp<real> t(h->main.s1);
  real *dlx = t.out(lx, (size_t)count * (N - 1) * n), *dph = t.out(Phix, (size_t)count * n);
  // one launch per run of problems of the same group
  if (t.e == hipSuccess)
    for_runs(first, count, [&](int b) { return h->plan.lid[b]; }, [&](int r0, int nb) {
      const size_t o = (size_t)(r0 - first);
      t.e = launch_cost_grad(h->sp, h->d, h->plan.lid[r0], phase, N, r0, nb, dlx + o * (N - 1) * n,
                             dph + o * n, h->main.s1);
      return t.e != hipSuccess;
    });
  if (t.fetch() != hipSuccess) return dev_fail("mhpc_get_cost_gradients", t.e);
  return MHPC_OK;
}

// The phase-buffer store of the receding-horizon loop, [B][spmax][nbk][SREC], zeroed at its
// first use after an initialize (the reference's memory_reset of its phase buffers); sized for
// the current layouts (buffers of N_TIMESTEPS_MAX = 110 knots, or the longest phase).
// The store's shape as ensure_store makes it (or has made it): knots a buffer, buffers a problem.
static void store_shape(const Handle* h, int* nbk_out, int* spmax_out) {
  int nbk = h->nbk, spmax = h->spmax;
  if (!h->store_valid) {
    nbk = kPhaseBufKnots;
    for (const Layout& L : h->plan.lays)
      for (int p = 0; p < L.P; ++p) nbk = std::max(nbk, L.N[p]);
    spmax = h->sp.pmax;
  }
  *nbk_out = nbk;
  *spmax_out = spmax;
}
static int ensure_store(Handle* h) {
  if (h->store_valid) return MHPC_OK;
  int nbk, spmax;
  store_shape(h, &nbk, &spmax);
  const size_t bytes = (size_t)h->sp.B * spmax * nbk * kStoreRec * sizeof(real);
  if (!h->store.get() || nbk != h->nbk || spmax != h->spmax) {
    h->store.reset();  // (before the new one is allocated, as ever: the two never coexist)
    HIPCHK(h->store.alloc(bytes / sizeof(real)));
    h->nbk = nbk;
    h->spmax = spmax;
  }
  HIPCHK(hipMemsetAsync(h->store.get(), 0, bytes, h->main.s1));
  h->store_valid = true;
  return MHPC_OK;
}

static int check_gaits(int n_gaits, const mhpc_gait* gaits) {
  if (n_gaits < 1 || n_gaits > MAXL) return fail(MHPC_ERR_INVALID, "n_gaits must be 1..MHPC_MAX_LAYOUTS");
  for (int gi = 0; gi < n_gaits; ++gi) {
    const mhpc_gait& g = gaits[gi];
    if (g.n_modes < 1 || g.n_modes > MHPC_MAX_PHASES)
      return fail(MHPC_ERR_INVALID, "gait needs 1..16 modes");
    for (int i = 0; i < g.n_modes; ++i)
      if (g.modes[i] < 1 || g.modes[i] > 4) return fail(MHPC_ERR_INVALID, "gait mode out of range");
  }
  return MHPC_OK;
}

// MHPCLocomotion::update_problem (MHPCLocomotion.cpp:107-158) per problem: problem b takes
// steps[b] gait steps (each: rotate the WB and SRB phase buffers by one, advance the gait by
// one mode, recompute mode sequence and knot counts -- Gait.h:48-77); then every problem's
// references are regenerated from the current x0 (mhpc_set_x0) and its AL / ReB parameters
// re-initialised.  The rotated nominal trajectories and gains are the warm start of the next
// mhpc_solve, whose first forward_sweep(0) is then a real rollout.  Problems whose layouts
// change move to the group of their new layout and their parameter set.
int api_update_problems(Handle* h, int n_gaits, const mhpc_gait* gaits, const int32_t* gait_of,
                        const int32_t* steps) {
  if (!h || !gaits) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "mhpc_initialize must precede mhpc_update_problem");
  if (int rc = check_gaits(n_gaits, gaits)) return rc;
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_store(h);
  if (rc) return rc;
  const int B = h->sp.B;
  std::vector<ProbLayout> npl = h->pl;
  std::vector<int> ncm = h->cmode;
  for (int b = 0; b < B; ++b) {
    const int gi = gait_of ? gait_of[b] : 0;
    if (gi < 0 || gi >= n_gaits) return fail(MHPC_ERR_INVALID, "gait index out of range");
    const int ns = steps ? steps[b] : 1;
    if (ns < 0 || ns > 1024) return fail(MHPC_ERR_INVALID, "steps must be 0..1024");
    PLANCHK(advance_gait, npl[b], ncm[b], gaits[gi], ns, h->nbk);
  }
  // phases write through to their buffers in the reference: save the current layouts (also when
  // the regrouping below is refused, as ever: the rows are the current solution's either way)
  HIPCHK(launch_store(h->sp, h->d, h->store.get(), h->nbk, h->spmax, 1, h->main.s1));
  GroupPlan plan;
  const char* msg = nullptr;
  if ((rc = plan_groups(npl, h->pset_of, plan, &msg))) {  // too many layouts: the old ones stay
    (void)hipStreamSynchronize(h->main.s1);
    return fail(rc, msg);
  }
  if ((rc = commit_groups(h, std::move(plan), false, &npl))) return rc;
  h->cmode = ncm;
  for (int b = 0; b < B; ++b)
    if ((steps ? steps[b] : 1) > 0) h->led.stepped(b);
  HIPCHK(launch_reset(h->sp, h->d, h->main.s1));  // refs from x0, AL/ReB init, nom_slot = 0
  if (own_init_values(h)) HIPCHK(launch_init_params(h->sp, h->d, 0, h->main.s1));
  HIPCHK(launch_store(h->sp, h->d, h->store.get(), h->nbk, h->spmax, 0, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  h->need_full = true;
  mark_current(h);
  return MHPC_OK;
}

int api_update_problem(Handle* h, const mhpc_gait* gait) {
  return api_update_problems(h, 1, gait, nullptr, nullptr);
}

// ---- per-problem ticks (mhpc_tick_problems) ---------------------------------------------------
// In the reference every robot is its own MHPCLocomotion and ticks when its own gait mode ends:
// set_initial_condition + update_problem (MHPCLocomotion.cpp:107-158) + solve_mhpc (:167-195), and
// no other robot notices.  Here: the listed problems take their x0 rows and gait steps, their
// references and AL / ReB state are regenerated from their current commands, and the solve
// schedule runs over them alone (a Scope of the list); each comes out bit for bit as after
// mhpc_set_x0 + mhpc_update_problems + mhpc_solve in a handle of its own, and every other
// problem's device records stay bit for bit.  Like mhpc_reset_problems it never re-strides or
// reallocates; everything that can refuse the call is decided on working copies before the handle
// or the device is touched.  Device work is proportional to n (but the one-off zeroing of the
// phase-buffer store); the host plan and the group-table upload stay O(batch) and are skipped
// when no listed problem takes a step.
int api_tick_problems(Handle* h, int n, const int32_t* problems, const double* x0, int n_gaits,
                      const mhpc_gait* gaits, const int32_t* gait_of, const int32_t* steps,
                      int32_t* status, float* ms) {
  if (!h || !problems) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "mhpc_initialize must precede mhpc_tick_problems");
  if (!h->solved)
    return fail(MHPC_ERR_STATE, "mhpc_solve must precede mhpc_tick_problems (the last batch-wide step was no solve)");
  if (h->params_changed) return fail(MHPC_ERR_STATE, kParamsPending);
  const int B = h->sp.B;
  ProblemList listed;
  PLANCHK(listed.begin, n, B, false);
  bool any_step = false;
  for (int i = 0; i < n; ++i) {
    PLANCHK(listed.add, problems[i]);
    const int ns = steps ? steps[i] : 1;
    if (ns < 0 || ns > 1024) return fail(MHPC_ERR_INVALID, "steps must be 0..1024");
    any_step = any_step || ns > 0;
  }
  if (!gaits && any_step) return fail(MHPC_ERR_INVALID, "gaits may be null only when every step is 0");
  int rc;
  if (gaits && (rc = check_gaits(n_gaits, gaits))) return rc;
  for (int i = 0; gaits && gait_of && i < n; ++i)
    if (gait_of[i] < 0 || gait_of[i] >= n_gaits) return fail(MHPC_ERR_INVALID, "gait index out of range");
  const int r = x0_row_of(h->plan);
  for (size_t i = 0; x0 && i < (size_t)n * r; ++i)
    if (!std::isfinite(x0[i])) return fail(MHPC_ERR_INVALID, "x0 must be finite");
  // the listed problems' gait steps on working copies; the arrays stay as they are, so each new
  // layout must fit the knot stride and the phase buffers (as the store is, or will be made)
  int nbk, spmax;
  store_shape(h, &nbk, &spmax);
  std::vector<ProbLayout> npl;
  std::vector<int> ncm;
  GroupPlan plan;
  if (any_step) {
    npl = h->pl;
    ncm = h->cmode;
    for (int i = 0; i < n; ++i) {
      const int b = problems[i], ns = steps ? steps[i] : 1;
      if (ns == 0) continue;
      PLANCHK(advance_gait, npl[b], ncm[b], gaits[gait_of ? gait_of[i] : 0], ns, nbk);
      PLANCHK(fits_arrays, npl[b], h->sp.NK, true, nbk, spmax, false);
    }
    PLANCHK(plan_groups, npl, h->pset_of, plan);  // too many groups: nothing changed
  }
  const GroupPlan& np = any_step ? plan : h->plan;
  // the scope: the list by its groups after the commit; fresh (mhpc_reset_problems) and no step:
  // the first forward_sweep(0) stays the cost evaluation
  std::vector<char> fr(B, 0);
  for (int i = 0; i < n; ++i) fr[problems[i]] = h->led.fresh(problems[i]) && (steps ? steps[i] : 1) == 0;
  const std::vector<int> list(problems, problems + n);
  const SolveScope ss = solve_scope(np, list, fr);
  std::vector<real> rows;  // in list order, padded as mhpc_set_x0 pads them (the plan before the commit)
  if (x0) rows = pack_rows<real>(h->plan, n, 1, x0, 0, problems);
  // ---- nothing of the handle or the device has changed up to here ----
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  HIPCHK(h->evt0.ensure(EV_TIMING));
  HIPCHK(h->evt1.ensure(EV_TIMING));
  DevTemp<int> ti(h->main.s1);
  DevTemp<real> tr(h->main.s1);
  const int* dlist = ti.in(std::vector<int>(list));
  const int* dorder = ti.in(std::vector<int>(ss.order));
  int* dstatus = status ? ti.alloc(n) : nullptr;
  const real* drows = rows.empty() ? nullptr : tr.in(std::move(rows));
  if (ti.e != hipSuccess) return dev_fail("mhpc_tick_problems", ti.e);
  if (tr.e != hipSuccess) return dev_fail("mhpc_tick_problems", tr.e);
  // from here a failure leaves the listed problems undefined (as a failed mhpc_reset_problems);
  // nothing of the handle's may stay queued behind it
  auto run = [&]() -> int {
    HIPCHK(hipEventRecord(h->evt0, h->main.s1));
    if (drows) HIPCHK(launch_scatter_x0(h->d, n, dlist, drows, h->main.s1));
    if (int rc = ensure_store(h)) return rc;
    // phases write through to their buffers in the reference: the listed problems' current
    // solutions under their layouts before the commit
    HIPCHK(launch_store_list(h->sp, h->d, n, dlist, h->store.get(), h->nbk, h->spmax, 1, h->main.s1));
    if (any_step) {
      if (int rc = commit_groups(h, std::move(plan), true, &npl)) return rc;
      for (int i = 0; i < n; ++i) h->cmode[problems[i]] = ncm[problems[i]];
    }
    Scope sc = make_scope(h, &ss, dorder, scope_caps(h->otab, list.data(), n), true);
    HIPCHK(launch_reset(sc.sp, sc.d, h->main.s1));  // refs from x0 and the command, AL/ReB init, nom_slot = 0
    if (own_init_values(h)) HIPCHK(launch_init_params(sc.sp, sc.d, 0, h->main.s1));
    HIPCHK(launch_store_list(h->sp, h->d, n, dlist, h->store.get(), h->nbk, h->spmax, 0, h->main.s1));
    HIPCHK(hipEventRecord(h->ev0, h->main.s1));
    if (int rc = solve_async(h, sc)) return rc;
    HIPCHK(hipEventRecord(h->ev1, h->main.s1));
    if (dstatus) HIPCHK(launch_status_list(h->d, n, dlist, dstatus, h->main.s1));
    HIPCHK(hipEventRecord(h->evt1, h->main.s1));
    HIPCHK(hipMemcpyAsync(h->gcnt, h->dcnt.get(), (size_t)sc.sp.ngrp * NCNT * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, h->main.s1));
    if (dstatus)
      HIPCHK(hipMemcpyAsync(status, dstatus, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->main.s1));
    HIPCHK(hipStreamSynchronize(h->main.s1));
    if (ms) HIPCHK(hipEventElapsedTime(ms, h->evt0, h->evt1));
    return account_solve(h, sc);
  };
  rc = run();
  // the listed problems have their references and their solve, whatever came of it: no longer
  // fresh, no command pending
  h->led.ticked(n, problems);
  if (rc) drain({h->main.s3, h->main.s2, h->main.s1});
  return rc;
}

// Floor of the knot stride of the packed arrays: a fleet created at one gait point can then tick
// into a longer layout (mhpc_tick_problems never re-strides).  Before mhpc_initialize only: the
// arrays hold nothing yet, so the stride is set here and kept by every later commit that may
// re-stride (commit_groups).
int api_reserve_knots(Handle* h, int knots) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  if (h->initialized) return fail(MHPC_ERR_STATE, "mhpc_reserve_knots must precede mhpc_initialize");
  if (knots < 1 || knots > MHPC_MAX_KNOTS) return fail(MHPC_ERR_INVALID, "knots must be 1..MHPC_MAX_KNOTS");
  HIPCHK(hipSetDevice(h->device));
  const int NK = std::max(h->plan.NK, knots);
  if (int rc = ensure_knot_arrays(h, NK)) return rc;
  h->sp.NK = NK;
  h->nk_floor = knots;
  return MHPC_OK;
}

// Per-problem phase layouts (the batch axis over gait schedules): problem b gets
// descs[lop[b]] with identity phase buffers; the handle is uninitialised afterwards.
int api_set_layouts(Handle* h, int n_desc, const mhpc_problem_desc* descs, const int32_t* lop) {
  if (!h || !descs) return fail(MHPC_ERR_INVALID, "null argument");
  if (n_desc < 1 || n_desc > MAXL) return fail(MHPC_ERR_INVALID, "n_desc must be 1..MHPC_MAX_LAYOUTS");
  for (int i = 0; i < n_desc; ++i) PLANCHK(check_layout_desc, descs[i], h->desc);
  const int B = h->sp.B;
  for (int b = 0; lop && b < B; ++b)
    if (lop[b] < 0 || lop[b] >= n_desc) return fail(MHPC_ERR_INVALID, "layout index out of range");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  std::vector<ProbLayout> npl(B);
  for (int b = 0; b < B; ++b) npl[b] = ProbLayout{norm_desc(descs[lop ? lop[b] : b % n_desc]), 0, 0};
  GroupPlan plan;
  PLANCHK(plan_groups, npl, h->pset_of, plan);  // too many layouts or groups: the old ones stay
  if (int rc = commit_groups(h, std::move(plan), false, &npl)) return rc;
  for (int b = 0; b < B; ++b) h->cmode[b] = h->pl[b].desc.mode_seq[0];
  h->store_valid = false;
  h->initialized = false;
  h->solved = false;
  h->x0_set = false;  // the x0 row length may have changed
  return MHPC_OK;
}

// The device half of mhpc_reset_problems: ss is the scope of the listed problems (its order: by
// group, then problem number), rows their padded x0 rows in that order (empty: the device rows
// stay).  The list-driven memory_reset runs on the second stream beside the warm start, as in
// initialize_async; k_init and k_init_params are the batch's own kernels over the scope's
// restricted parameters (make_scope).  Every launch counts as k_init under profiling.
static int reset_launches(Handle* h, const SolveScope& ss, std::vector<real>&& rows) {
  const int n = ss.size();
  DevTemp<int> ti(h->main.s1);
  DevTemp<real> tr(h->main.s1);
  const int* dlist = ti.in(std::vector<int>(ss.order));
  const real* drows = rows.empty() ? nullptr : tr.in(std::move(rows));
  if (ti.e != hipSuccess) return dev_fail("mhpc_reset_problems", ti.e);
  if (tr.e != hipSuccess) return dev_fail("mhpc_reset_problems", tr.e);
  const Scope rs = make_scope(h, &ss, dlist, ScopeCaps(), false);
  HIPCHK(hipEventRecord(h->main.fork, h->main.s1));
  HIPCHK(hipStreamWaitEvent(h->main.s2, h->main.fork, 0));
  LAUNCH_ON(h, K_INIT, h->main.s2,
            launch_reset_list(h->sp, h->d, n, dlist, h->store_valid ? h->store.get() : nullptr, h->nbk,
                              h->spmax, h->main.s2));
  HIPCHK(hipEventRecord(h->main.join, h->main.s2));
  if (drows) LAUNCH(h, K_INIT, launch_scatter_x0(h->d, n, dlist, drows, h->main.s1));
  LAUNCH(h, K_INIT, launch_init(rs.sp, rs.d, h->main.s1));
  // (k_init wrote the AL / ReB initial values of problem 0's set)
  if (own_init_values(h)) LAUNCH(h, K_INIT, launch_init_params(rs.sp, rs.d, 1, h->main.s1));
  HIPCHK(hipStreamWaitEvent(h->main.s1, h->main.join, 0));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  return MHPC_OK;
}

// MHPCLocomotion::initialization() (MHPCLocomotion.cpp:47-53: memory_reset, build_problem,
// generate_ref, warmstart) of the listed problems only: each comes out as mhpc_initialize leaves
// a problem (its own command and parameter set, the given x0 row or its current one, identity
// phase buffers, optionally another descriptor); every other problem's device records stay bit
// for bit, so the knot stride never changes here and a descriptor that does not fit the arrays
// as they are is refused.  The handle's call-order flags stay as they are.
int api_reset_problems(Handle* h, int n, const int32_t* problems, const double* x0, int n_desc,
                       const mhpc_problem_desc* descs, const int32_t* desc_of) {
  if (!h || !problems) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "mhpc_initialize must precede mhpc_reset_problems");
  const int B = h->sp.B;
  ProblemList listed;  // (listed.at: a listed problem's place in the list)
  PLANCHK(listed.begin, n, B, false);
  for (int i = 0; i < n; ++i) PLANCHK(listed.add, problems[i]);
  if (!descs && n_desc != 0) return fail(MHPC_ERR_INVALID, "n_desc without descriptors");
  if (descs && (n_desc < 1 || n_desc > MAXL))
    return fail(MHPC_ERR_INVALID, "n_desc must be 1..MHPC_MAX_LAYOUTS");
  for (int i = 0; i < n_desc; ++i) PLANCHK(check_layout_desc, descs[i], h->desc);
  for (int i = 0; descs && desc_of && i < n; ++i)
    if (desc_of[i] < 0 || desc_of[i] >= n_desc) return fail(MHPC_ERR_INVALID, "layout index out of range");
  const int r = x0_row_of(h->plan);
  std::vector<ProbLayout> npl = h->pl;
  for (int i = 0; i < n; ++i) {
    ProbLayout& q = npl[problems[i]];
    if (descs) q.desc = norm_desc(descs[desc_of ? desc_of[i] : i % n_desc]);
    q.rot_wb = q.rot_fb = 0;
    // the arrays stay as they are: the layout must fit the knot stride and the phase buffers
    PLANCHK(fits_arrays, q, h->sp.NK, h->store_valid, h->nbk, h->spmax, false);
  }
  if (x0_row_of(npl) != r) return fail(MHPC_ERR_INVALID, "the x0 row width would change");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  GroupPlan plan;
  PLANCHK(plan_groups, npl, h->pset_of, plan);  // too many groups: nothing changed
  int rc = commit_groups(h, std::move(plan), true, &npl);
  if (rc) return rc;
  // the listed problems by group under the new plan, their x0 rows in that order
  const SolveScope ss = solve_scope(h->plan, std::vector<int>(problems, problems + n), {});
  std::vector<real> rows;
  if (x0) rows = pack_rows<real>(h->plan, n, 1, x0, 0, ss.order.data(), listed.at.data());
  for (int b : ss.order) {
    h->cmode[b] = h->pl[b].desc.mode_seq[0];
    h->kbytes[K_INIT] += h->plan.bym[h->plan.lid[b]].init + (own_init_values(h) ? 4 * MAXP * kB : 0.0);
    h->led.reset(b, no_al_iteration(h->otab.rec[h->otab.of[b]]));
  }
  rc = reset_launches(h, ss, std::move(rows));
  if (rc) {  // nothing of the handle's may stay queued behind a failed launch
    drain({h->main.s2, h->main.s1});
    return rc;
  }
  return collect_profile(h);
}

// ---- copies of live problems (mhpc_copy_problems, mhpc_restore_problems) ------------------------
static CopySide copy_side(const Handle* h) {
  return CopySide{h->d, h->store_valid ? h->store.get() : nullptr, h->sp.NK, h->sp.nslot, h->nbk, h->spmax};
}

// The host state of one source problem that travels with a copy -- and, byte for byte, the entry
// record of a snapshot blob (fixed-width members, no padding, no pointers).
struct SrcProblem {
  ProbLayout pl;  // layout with its buffer rotation
  int32_t cmode, fresh, open, reserved;  // gait point; the ledger's marks
  double cmd[2];
  mhpc_hsddp_option opt;
  CostParams cw;
};
static_assert(sizeof(SrcProblem) == sizeof(ProbLayout) + 4 * sizeof(int32_t) + 2 * sizeof(double) +
                                        sizeof(mhpc_hsddp_option) + sizeof(CostParams) &&
                  sizeof(ProbLayout) == sizeof(mhpc_problem_desc) + 2 * sizeof(int),
              "a snapshot entry has no padding");
static SrcProblem src_problem(const Handle* s, int a) {
  SrcProblem q;
  memset(&q, 0, sizeof q);
  q.pl = s->pl[a];
  q.cmode = s->cmode[a];
  q.fresh = s->led.fresh(a);
  q.open = s->led.open(a);
  q.cmd[0] = s->cmd[2 * (size_t)a];
  q.cmd[1] = s->cmd[2 * (size_t)a + 1];
  q.opt = s->otab.rec[s->otab.of[a]];
  q.cw = s->psets[s->pset_of[a]];
  return q;
}

// What a copy compares and takes, whether its source is a live handle or a snapshot blob.
struct CopySource {
  const char* call;   // the entry point, for messages
  bool blob;          // a snapshot: a copy that covers the whole destination adopts its call-order point
  double alpha;
  int nslot, x0_row;
  bool sweep32, initialized, pending, need_full, solved, has_store;
  std::vector<SrcProblem> p;  // the listed source problems, in list order
};
static CopySource source_of(const Handle* s, const char* call) {
  return CopySource{call, false, s->opt.alpha, s->sp.nslot, x0_row_of(s->plan), s->sweep_bits == 32,
                    s->initialized, pending(s), s->need_full, s->solved, s->store_valid, {}};
}
// The device part of a copy, which differs between the two: one launch out of the source handle's
// arrays, or rounds through the staging buffers of a blob.
struct CopyMover {
  virtual ~CopyMover() {}
  // everything that can fail while the destination can still go back: allocations, uploads, the
  // order against the source's stream (dst's arrays and store are final here)
  virtual hipError_t prepare(Handle* d, const int32_t* dp, int n) = 0;
  // the copy of every pair, queued and waited for; ms: device time of its launches
  virtual hipError_t run(Handle* d, float* ms) = 0;
};

// In the reference a controller is an object and a copy of it is a copy of the object: the
// destination problems become the source problems as they stand -- nominal and trial slots,
// K / du / G, partials, impact Jacobians, solver state, x0 row, references, command, parameter set,
// layout with its buffer rotation, gait point, phase-buffer rows -- inside one handle or between
// two of one device, or out of a snapshot blob.  Like mhpc_reset_problems it never re-strides or
// reallocates the destination's packed arrays and leaves every other problem's records where they
// are; everything that can refuse the call is checked before anything changes (a device error,
// unlike a refusal, can leave the destination problems undefined, as for a reset).  dp: n checked
// destination problems, none twice.  All the handle's streams are idle when the call returns.
static int copy_into(Handle* d, const int32_t* dp, int n, const CopySource& src, CopyMover& mv, float* ms) {
  // the line-search grid (alpha, nslot: the arrays' shape) is the handle's; a source problem's
  // option record travels with it, as an index into dst's table -- the copy never adds a record
  // to it (that would change dst's launch schedule), so the record must be one of dst's already
  // (inside one handle that is the source's own slot: equal records share one)
  if (memcmp(&d->opt.alpha, &src.alpha, sizeof(double)) != 0 || d->sp.nslot != src.nslot)
    return fail(MHPC_ERR_INVALID, "the handles' mhpc_hsddp_option differ");
  std::vector<int> nslot_of(n);  // dst's slot of each source problem's record
  for (int i = 0; i < n; ++i) {
    nslot_of[i] = d->otab.find(src.p[i].opt);
    if (nslot_of[i] < 0)
      return fail(MHPC_ERR_INVALID,
                  "the handles' mhpc_hsddp_option differ: a source problem's option set is none of the destination's");
  }
  // the one kernel variant that changes results: the sweep's arithmetic (0 and 64 are both double)
  if ((d->sweep_bits == 32) != src.sweep32)
    return fail(MHPC_ERR_INVALID, "the handles' backward-sweep arithmetic (MHPC_VARIANT_SWEEP_BITS) differs");
  // the destination's arrays stay as they are: every source layout must fit them
  const int r = x0_row_of(d->plan);
  if (src.x0_row != r) return fail(MHPC_ERR_INVALID, "the handles' x0 row widths differ");
  std::vector<ProbLayout> npl = d->pl;
  std::vector<CostParams> nsets = d->psets;
  std::vector<int> nof = d->pset_of;
  for (int i = 0; i < n; ++i) {
    const ProbLayout& q = src.p[i].pl;
    PLANCHK(fits_arrays, q, d->sp.NK, d->store_valid, d->nbk, d->spmax, true);
    npl[dp[i]] = q;
    nof[dp[i]] = (int)nsets.size();  // the source's set, merged below with the ones it equals
    nsets.push_back(src.p[i].cw);
  }
  if (x0_row_of(npl) != r) return fail(MHPC_ERR_INVALID, "the x0 row width would change");
  if (!d->initialized || !src.initialized)
    return fail(MHPC_ERR_STATE, std::string("mhpc_initialize must precede ") + src.call);
  if (pending(d) || src.pending)
    return fail(MHPC_ERR_STATE,
                "commands or parameters pending: call mhpc_initialize or mhpc_update_problem first");
  // a snapshot that replaces every problem of the destination brings its point of the call order
  const bool adopt = src.blob && n == d->sp.B;
  if (!adopt && (d->need_full != src.need_full || d->solved != src.solved))
    return fail(MHPC_ERR_STATE, "the handles are at different points of the call order");
  merge_sets(nsets, nof);
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->main.s1));
  GroupPlan plan;
  PLANCHK(plan_groups, npl, nof, plan);  // too many groups: nothing changed
  // Until the launch is queued the destination can go back to what it was: the commit swaps its
  // plan, layouts and sets for the new ones (plan, npl, nsets, nof then hold the old ones), its
  // store is created, the lists uploaded -- and on any failure the old ones are committed again.
  // The per-problem host entries change only after that.
  int rc = commit_groups(d, std::move(plan), true, &npl, &nsets, &nof);
  if (rc) return rc;
  // a source with phase buffers gives the destination its own, as its first update would (an
  // empty store of the new layouts' shape, which the old layouts fit as well)
  if (src.has_store && (rc = ensure_store(d))) {
    (void)commit_groups(d, std::move(plan), true, &npl, &nsets, &nof);
    return rc;
  }
  // the (destination problem, option slot) entries of the option hand-over
  std::vector<int> ent(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    ent[2 * (size_t)i] = dp[i];
    ent[2 * (size_t)i + 1] = nslot_of[i];
  }
  DevTemp<int> t(d->main.s1);
  const int* dent = t.in(std::move(ent));
  if (t.e == hipSuccess) t.e = mv.prepare(d, dp, n);
  if (t.e != hipSuccess) {  // nothing of the copy is queued yet
    drain({d->main.s2, d->main.s1});
    (void)commit_groups(d, std::move(plan), true, &npl, &nsets, &nof);
    return dev_fail(src.call, t.e);
  }
  for (int i = 0; i < n; ++i) {
    const SrcProblem& q = src.p[i];
    const int b = dp[i];
    d->cmode[b] = q.cmode;
    d->cmd[2 * (size_t)b] = q.cmd[0];
    d->cmd[2 * (size_t)b + 1] = q.cmd[1];
    d->led.copied(b, q.fresh != 0, q.open != 0);
  }
  float el = 0;
  t.e = mv.run(d, &el);
  // the option index of the destinations (their rewritten option fields came with the state)
  if (t.e == hipSuccess) t.e = launch_set_options(d->d, d->own.oid.get(), n, dent, 0, d->main.s1);
  if (t.e == hipSuccess) t.e = hipStreamSynchronize(d->main.s1);
  if (t.e != hipSuccess) {
    // a failed launch: the destination problems are undefined (as after a failed reset); nothing
    // of the handle's may stay queued behind it
    drain({d->main.s2, d->main.s1});
    return dev_fail(src.call, t.e);
  }
  // the host table follows the device index once the launches have succeeded (a record the
  // destinations were the last to use is dropped; problem 0's may have changed)
  for (int i = 0; i < n; ++i) {
    const int b = dp[i];
    --d->otab.use[d->otab.of[b]];
    ++d->otab.use[nslot_of[i]];
    d->otab.of[b] = nslot_of[i];
  }
  mirror_option0(d);
  if (adopt) {
    d->need_full = src.need_full;
    d->solved = src.solved;
  }
  if (ms) *ms = el;
  return MHPC_OK;
}

// One list-driven launch (mhpc_copy.hip) on the destination's stream, after an event on the
// source's.
struct HandleMover : CopyMover {
  Handle* s;
  const int32_t* sp;
  DevTemp<int> t;
  const int* dpairs = nullptr;
  int n = 0, nblk = 0;
  CopySide cs, cd;
  HandleMover(Handle* src, const int32_t* src_problems, hipStream_t q) : s(src), sp(src_problems), t(q) {}
  hipError_t prepare(Handle* d, const int32_t* dp, int n_) override {
    n = n_;
    cs = copy_side(s);
    cd = copy_side(d);
    // the pair list and, behind it, the (run, chunk) table of one pair: one upload
    nblk = copy_block_table(cs, cd, nullptr);
    std::vector<int> pairs(2 * (size_t)n + nblk);
    for (int i = 0; i < n; ++i) {
      pairs[2 * (size_t)i] = sp[i];
      pairs[2 * (size_t)i + 1] = dp[i];
    }
    copy_block_table(cs, cd, pairs.data() + 2 * (size_t)n);
    dpairs = t.in(std::move(pairs));
    if (t.e == hipSuccess && s != d) {
      t.e = hipEventRecord(s->main.fork, s->main.s1);
      if (t.e == hipSuccess) t.e = hipStreamWaitEvent(d->main.s1, s->main.fork, 0);
    }
    return t.e;
  }
  hipError_t run(Handle* d, float* ms) override {
    hipError_t e = hipEventRecord(d->ev0, d->main.s1);
    if (e == hipSuccess) e = launch_copy_problems(cs, cd, n, dpairs, nblk, dpairs + 2 * (size_t)n, d->main.s1);
    if (e == hipSuccess) e = hipEventRecord(d->ev1, d->main.s1);
    if (e == hipSuccess) e = hipStreamSynchronize(d->main.s1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, d->ev0, d->ev1);
    return e;
  }
};

int api_copy_problems(Handle* d, const int32_t* dp, Handle* s, const int32_t* sp_, int n, float* ms) {
  if (!d || !s || !dp || !sp_) return fail(MHPC_ERR_INVALID, "null argument");
  const int Bd = d->sp.B, Bs = s->sp.B;
  ProblemList dst;
  PLANCHK(dst.begin, n, Bd, true);
  for (int i = 0; i < n; ++i) {  // (an entry's ranges, source and destination, before "twice")
    if (sp_[i] < 0 || sp_[i] >= Bs) return fail(MHPC_ERR_INVALID, "problem out of range");
    PLANCHK(dst.add, dp[i]);
  }
  for (int i = 0; d == s && i < n; ++i)
    if (dst.at[sp_[i]] >= 0)
      return fail(MHPC_ERR_INVALID, "a problem is both a source and a destination");
  if (d->device != s->device) return fail(MHPC_ERR_INVALID, "the handles are on different devices");
  // (d == s: a source is no destination, so its entries are read before any of them changes)
  CopySource src = source_of(s, "mhpc_copy_problems");
  src.p.reserve(n);
  for (int i = 0; i < n; ++i) src.p.push_back(src_problem(s, sp_[i]));
  HandleMover mv(s, sp_, d->main.s1);
  return copy_into(d, dp, n, src, mv, ms);
}

// ---- snapshots of live problems (mhpc_snapshot_problems, mhpc_restore_problems) -----------------
// The serialised form of the copy above: header, entry table (SrcProblem records), payload
// (mhpc_snapshot_map.h).  A snapshot packs the listed problems through staging sides whose knot
// stride is the longest listed layout; a restore is copy_into with the blob as its source.
static constexpr size_t kSnapStageCap = (size_t)256 << 20;  // bytes of one staging buffer

static mhpc_copy::Sizes snap_sizes() {
  return mhpc_copy::Sizes{(int)sizeof(real), (int)sizeof(ProbState), (int)sizeof(BwsCarry)};
}
// The header of a snapshot of the listed (checked) problems of h.
static mhpc_snap::Header snap_header(const Handle* h, int n, const int32_t* problems) {
  mhpc_snap::Header o;
  memset(&o, 0, sizeof o);
  int NK = 1;
  for (int i = 0; i < n; ++i) {
    const mhpc_problem_desc& q = h->pl[problems[i]].desc;
    int nk = 0;
    for (int p = 0; p < q.n_wb + q.n_fb; ++p) nk += q.N[p];
    NK = std::max(NK, nk);
  }
  o.magic = mhpc_snap::MAGIC;
  o.version = mhpc_snap::FORMAT_VERSION;
  o.header_bytes = sizeof o;
  o.n_entries = n;
  o.entry_bytes = sizeof(SrcProblem);
  o.precision = sizeof(real) == 4 ? 32 : 64;
  o.elem_bytes = sizeof(real);
  o.sizeof_state = sizeof(ProbState);
  o.sizeof_carry = sizeof(BwsCarry);
  o.KS = KS;
  o.PS = PS;
  o.PS_JAC = PS_JAC;
  o.SREC = kStoreRec;
  o.MAXP = MAXP;
  o.nslot = h->sp.nslot;
  memcpy(&o.alpha_bits, &h->opt.alpha, sizeof(double));
  o.sweep32 = h->sweep_bits == 32;
  o.x0_row = x0_row_of(h->plan);
  o.NK = std::min(NK, h->sp.NK);
  o.nbk = h->store_valid ? h->nbk : 0;
  o.spmax = h->store_valid ? h->spmax : 0;
  o.need_full = h->need_full;
  o.solved = h->solved;
  o.payload_entry_bytes = mhpc_snap::entry_payload_bytes(mhpc_snap::dims_of(o), snap_sizes());
  o.total_bytes = sizeof o + (size_t)n * (o.entry_bytes + o.payload_entry_bytes);
  return o;
}
static int snap_list(const Handle* h, int n, const int32_t* problems) {
  if (!h || !problems) return fail(MHPC_ERR_INVALID, "null argument");
  ProblemList l;
  PLANCHK(l.begin, n, h->sp.B, false);
  for (int i = 0; i < n; ++i) PLANCHK(l.add, problems[i]);
  return MHPC_OK;
}
// A blob this build can read: the format's own checks, then this instantiation's sizes.
static int snap_open(const void* blob, int64_t bytes, mhpc_snap::Header* hd) {
  if (!blob || bytes < 0) return fail(MHPC_ERR_INVALID, "null snapshot blob");
  if (const char* why = mhpc_snap::validate(blob, (size_t)bytes, hd)) return fail(MHPC_ERR_INVALID, why);
  if (hd->precision != (sizeof(real) == 4 ? 32u : 64u) || hd->elem_bytes != sizeof(real))
    return fail(MHPC_ERR_INVALID, "the snapshot's precision differs from the handle's");
  if (hd->sizeof_state != sizeof(ProbState) || hd->sizeof_carry != sizeof(BwsCarry))
    return fail(MHPC_ERR_INVALID, "snapshot of another build: sizeof(ProbState) / sizeof(BwsCarry) differ");
  if (hd->KS != (unsigned)KS || hd->PS != (unsigned)PS || hd->PS_JAC != (unsigned)PS_JAC ||
      hd->SREC != (unsigned)kStoreRec || hd->MAXP != (unsigned)MAXP || hd->entry_bytes != sizeof(SrcProblem))
    return fail(MHPC_ERR_INVALID, "snapshot of another build: record widths (KS, PS, PS_JAC, SREC, MAXP) differ");
  if (const char* why = mhpc_snap::consistent(*hd)) return fail(MHPC_ERR_INVALID, why);
  return MHPC_OK;
}

int api_snapshot_size(Handle* h, int n, const int32_t* problems, int64_t* bytes) {
  if (!bytes) return fail(MHPC_ERR_INVALID, "null argument");
  if (int rc = snap_list(h, n, problems)) return rc;
  *bytes = (int64_t)snap_header(h, n, problems).total_bytes;
  return MHPC_OK;
}

// The two staging buffers of a snapshot or restore and the events that time its launches; the
// rounds alternate between the handle's two streams, each with a buffer of its own, so a round's
// launch runs beside the other round's copies and a buffer is reused in stream order.
struct SnapStage {
  DevArray<char> buf[2];
  std::vector<Event> ev;  // [rounds][2]
  hipError_t alloc(size_t bytes, int rounds) {
    for (int k = 0; k < (rounds > 1 ? 2 : 1); ++k)
      if (hipError_t e = buf[k].alloc(bytes)) return e;
    ev.resize(2 * (size_t)rounds);
    for (Event& x : ev)
      if (hipError_t e = x.create(EV_TIMING)) return e;
    return hipSuccess;
  }
  hipError_t elapsed(int rounds, float* ms) const {
    float sum = 0;
    for (int r = 0; r < rounds; ++r) {
      float el = 0;
      if (hipError_t e = hipEventElapsedTime(&el, ev[2 * (size_t)r], ev[2 * (size_t)r + 1])) return e;
      sum += el;
    }
    *ms = sum;
    return hipSuccess;
  }
};
static int snap_round(const Handle* h, size_t entry_bytes, int n) {
  return h->snap_round_req > 0 ? std::min(h->snap_round_req, n)
                               : mhpc_snap::default_round(entry_bytes, kSnapStageCap, n);
}

int api_snapshot_problems(Handle* h, int n, const int32_t* problems, void* blob, int64_t bytes, float* ms) {
  if (!blob) return fail(MHPC_ERR_INVALID, "null argument");
  if (int rc = snap_list(h, n, problems)) return rc;
  if (!h->initialized) return fail(MHPC_ERR_STATE, "mhpc_initialize must precede mhpc_snapshot_problems");
  if (pending(h))
    return fail(MHPC_ERR_STATE,
                "commands or parameters pending: call mhpc_initialize or mhpc_update_problem first");
  mhpc_snap::Header hd = snap_header(h, n, problems);
  if (bytes < (int64_t)hd.total_bytes)
    return fail(MHPC_ERR_INVALID, "snapshot buffer too small (mhpc_snapshot_size)");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  const int NK = hd.NK, nslot = hd.nslot, nbk = hd.nbk, spmax = hd.spmax;
  const int R = snap_round(h, hd.payload_entry_bytes, n), rounds = mhpc_snap::n_rounds(n, R);
  const CopySide cs = copy_side(h), cstage = snap_side(nullptr, R, NK, nslot, nbk, spmax);
  // the pair list (source problem, staging record) and behind it the (run, chunk) table of a pair
  const int nblk = copy_block_table(cs, cstage, nullptr);
  std::vector<int> pairs(2 * (size_t)n + nblk);
  for (int i = 0; i < n; ++i) {
    pairs[2 * (size_t)i] = problems[i];
    pairs[2 * (size_t)i + 1] = i % R;
  }
  copy_block_table(cs, cstage, pairs.data() + 2 * (size_t)n);
  DevTemp<int> t(h->main.s1);
  const int* dpairs = t.in(std::move(pairs));
  SnapStage st;
  if (t.e == hipSuccess) t.e = st.alloc(snap_stage_bytes(R, NK, nslot, nbk, spmax), rounds);
  if (t.e == hipSuccess) t.e = hipStreamSynchronize(h->main.s1);  // the lists are up before s2 reads them
  char* payload = (char*)blob + sizeof hd + (size_t)n * sizeof(SrcProblem);
  for (int r = 0; t.e == hipSuccess && r < rounds; ++r) {
    int e0, cnt;
    mhpc_snap::round_of(n, R, r, &e0, &cnt);
    const hipStream_t q = r & 1 ? h->main.s2 : h->main.s1;
    void* buf = st.buf[r & 1].get();
    t.e = hipEventRecord(st.ev[2 * (size_t)r], q);
    if (t.e == hipSuccess)
      t.e = launch_copy_problems(cs, snap_side(buf, R, NK, nslot, nbk, spmax), cnt, dpairs + 2 * (size_t)e0,
                                 nblk, dpairs + 2 * (size_t)n, q);
    if (t.e == hipSuccess) t.e = hipEventRecord(st.ev[2 * (size_t)r + 1], q);
    if (t.e == hipSuccess) t.e = snap_move(buf, R, NK, nslot, nbk, spmax, payload, n, e0, 0, cnt, true, q);
  }
  // after an error nothing more was queued; either way both streams are idle from here
  for (hipStream_t q : {(hipStream_t)h->main.s2, (hipStream_t)h->main.s1}) {
    const hipError_t e = hipStreamSynchronize(q);
    if (t.e == hipSuccess) t.e = e;
  }
  float el = 0;
  if (t.e == hipSuccess) t.e = st.elapsed(rounds, &el);
  if (t.e != hipSuccess) return dev_fail("mhpc_snapshot_problems", t.e);
  // header and entry table last: a blob with a valid header has its whole payload
  char* ent = (char*)blob + sizeof hd;
  for (int i = 0; i < n; ++i) {
    const SrcProblem q = src_problem(h, problems[i]);
    memcpy(ent + (size_t)i * sizeof q, &q, sizeof q);
  }
  hd.checksum = mhpc_snap::checksum_of(hd, ent);
  memcpy(blob, &hd, sizeof hd);
  if (ms) *ms = el;
  return MHPC_OK;
}

// Rounds of distinct blob entries through the staging buffers: upload, then unpack with the
// destination's strides (k_copy_problems out of the staging side).
struct BlobMover : CopyMover {
  mhpc_snap::Header hd;
  char* payload;
  const int32_t* entries;  // [n] entry of each destination (null: entry i)
  int R_req;
  DevTemp<int> t;
  SnapStage st;
  const int* dlists = nullptr;
  int R = 0, rounds = 0, nblk = 0, n = 0;
  std::vector<int> uniq;             // the distinct entries, ascending
  std::vector<int> first, count;     // [rounds] each round's pairs in the uploaded list
  CopySide cd;
  BlobMover(const mhpc_snap::Header& h, const void* blob, const int32_t* ent, int round_req, hipStream_t q)
      : hd(h), payload((char*)blob + sizeof(mhpc_snap::Header) + (size_t)h.n_entries * h.entry_bytes),
        entries(ent), R_req(round_req), t(q) {}
  CopySide stage(void* buf) const {
    return snap_side(buf, R, (int)hd.NK, (int)hd.nslot, (int)hd.nbk, (int)hd.spmax);
  }
  hipError_t prepare(Handle* d, const int32_t* dp, int n_) override {
    n = n_;
    auto entry = [&](int i) { return entries ? entries[i] : i; };
    for (int i = 0; i < n; ++i) uniq.push_back(entry(i));
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int nu = (int)uniq.size();
    R = R_req > 0 ? std::min(R_req, nu) : mhpc_snap::default_round(hd.payload_entry_bytes, kSnapStageCap, nu);
    rounds = mhpc_snap::n_rounds(nu, R);
    cd = copy_side(d);
    const CopySide cstage = stage(nullptr);
    nblk = copy_block_table(cstage, cd, nullptr);
    // the pairs (staging record, destination problem) round by round, then the block table
    std::vector<int> lists;
    lists.reserve(2 * (size_t)n + nblk);
    first.assign(rounds, 0);
    count.assign(rounds, 0);
    for (int r = 0; r < rounds; ++r) {
      first[r] = (int)lists.size() / 2;
      for (int i = 0; i < n; ++i) {
        const int u = (int)(std::lower_bound(uniq.begin(), uniq.end(), entry(i)) - uniq.begin());
        if (u / R != r) continue;
        lists.push_back(u % R);
        lists.push_back(dp[i]);
      }
      count[r] = (int)lists.size() / 2 - first[r];
    }
    lists.resize(2 * (size_t)n + nblk);
    copy_block_table(cstage, cd, lists.data() + 2 * (size_t)n);
    dlists = t.in(std::move(lists));
    if (t.e == hipSuccess)
      t.e = st.alloc(snap_stage_bytes(R, (int)hd.NK, (int)hd.nslot, (int)hd.nbk, (int)hd.spmax), rounds);
    if (t.e == hipSuccess) t.e = hipStreamSynchronize(d->main.s1);  // the lists are up before s2 reads them
    return t.e;
  }
  hipError_t run(Handle* d, float* ms) override {
    hipError_t e = hipSuccess;
    for (int r = 0; e == hipSuccess && r < rounds; ++r) {
      int u0, cnt;
      mhpc_snap::round_of((int)uniq.size(), R, r, &u0, &cnt);
      const hipStream_t q = r & 1 ? d->main.s2 : d->main.s1;
      void* buf = st.buf[r & 1].get();
      // consecutive entries of the round travel in one copy per array
      for (int a = 0; e == hipSuccess && a < cnt;) {
        int b = a + 1;
        while (b < cnt && uniq[u0 + b] == uniq[u0 + b - 1] + 1) ++b;
        e = snap_move(buf, R, (int)hd.NK, (int)hd.nslot, (int)hd.nbk, (int)hd.spmax, payload, (int)hd.n_entries,
                      uniq[u0 + a], a, b - a, false, q);
        a = b;
      }
      if (e == hipSuccess) e = hipEventRecord(st.ev[2 * (size_t)r], q);
      if (e == hipSuccess)
        e = launch_copy_problems(stage(buf), cd, count[r], dlists + 2 * (size_t)first[r], nblk,
                                 dlists + 2 * (size_t)n, q);
      if (e == hipSuccess) e = hipEventRecord(st.ev[2 * (size_t)r + 1], q);
    }
    // after an error nothing more was queued; either way both streams are idle from here
    for (hipStream_t q : {(hipStream_t)d->main.s2, (hipStream_t)d->main.s1}) {
      const hipError_t s = hipStreamSynchronize(q);
      if (e == hipSuccess) e = s;
    }
    if (e == hipSuccess) e = st.elapsed(rounds, ms);
    return e;
  }
};

int api_restore_problems(Handle* d, int n, const int32_t* dp, const void* blob, int64_t bytes,
                         const int32_t* entries, float* ms) {
  if (!d || !dp) return fail(MHPC_ERR_INVALID, "null argument");
  mhpc_snap::Header hd;
  if (int rc = snap_open(blob, bytes, &hd)) return rc;
  ProblemList dst;
  PLANCHK(dst.begin, n, d->sp.B, true);
  for (int i = 0; i < n; ++i) {
    const int e = entries ? entries[i] : i;
    if (e < 0 || e >= (int)hd.n_entries) return fail(MHPC_ERR_INVALID, "snapshot entry out of range");
    PLANCHK(dst.add, dp[i]);
  }
  double alpha;
  memcpy(&alpha, &hd.alpha_bits, sizeof alpha);
  CopySource src{"mhpc_restore_problems", true, alpha, (int)hd.nslot, (int)hd.x0_row, hd.sweep32 != 0,
                 true, false, hd.need_full != 0, hd.solved != 0, hd.spmax > 0, {}};
  src.p.resize(n);
  const char* ent = (const char*)blob + sizeof hd;
  for (int i = 0; i < n; ++i)
    memcpy(&src.p[i], ent + (size_t)(entries ? entries[i] : i) * sizeof(SrcProblem), sizeof(SrcProblem));
  // (the entries passed the checksum, but a descriptor is still checked like a caller's)
  for (int i = 0; i < n; ++i) {
    PLANCHK(check_desc, &src.p[i].pl.desc);
    const mhpc_problem_desc& q = src.p[i].pl.desc;
    int nk = 0;
    for (int p = 0; p < q.n_wb + q.n_fb; ++p) nk += q.N[p];
    if (nk > (int)hd.NK) return fail(MHPC_ERR_INVALID, "snapshot entry longer than the blob's knot stride");
  }
  BlobMover mv(hd, blob, entries, d->snap_round_req, d->main.s1);
  return copy_into(d, dp, n, src, mv, ms);
}

// Entry `entry` of a blob, on the host alone.
int api_snapshot_entry(const void* blob, int64_t bytes, int entry, mhpc_problem_desc* desc,
                       mhpc_hsddp_option* option, mhpc_cost_weights* w, mhpc_constraint_params* c) {
  mhpc_snap::Header hd;
  if (int rc = snap_open(blob, bytes, &hd)) return rc;
  if (entry < 0 || entry >= (int)hd.n_entries) return fail(MHPC_ERR_INVALID, "snapshot entry out of range");
  SrcProblem q;
  memcpy(&q, (const char*)blob + sizeof hd + (size_t)entry * sizeof q, sizeof q);
  if (desc) {
    *desc = q.pl.desc;
    desc->vel_cmd = q.cmd[0];
    desc->height_cmd = q.cmd[1];
  }
  if (option) *option = q.opt;
  if (w) get_weights(q.cw, *w);
  if (c) get_constraints(q.cw, *c);
  return MHPC_OK;
}
// ProbState::status of entries [first, first + count), from the payload.
int api_snapshot_status(const void* blob, int64_t bytes, int first, int count, int32_t* status) {
  if (!status) return fail(MHPC_ERR_INVALID, "null argument");
  mhpc_snap::Header hd;
  if (int rc = snap_open(blob, bytes, &hd)) return rc;
  if (first < 0 || count < 1 || first > (int)hd.n_entries - count)
    return fail(MHPC_ERR_INVALID, "snapshot entry out of range");
  const char* st = (const char*)blob + sizeof hd + (size_t)hd.n_entries * sizeof(SrcProblem) +
                   mhpc_snap::payload_off(mhpc_snap::dims_of(hd), snap_sizes(), mhpc_copy::A_ST, hd.n_entries);
  for (int i = 0; i < count; ++i) {
    ProbState s;
    memcpy(&s, st + (size_t)(first + i) * sizeof s, sizeof s);
    status[i] = s.status;
  }
  return MHPC_OK;
}

int api_get_problem_desc(Handle* h, int b, mhpc_problem_desc* desc) {
  if (!h || !desc) return fail(MHPC_ERR_INVALID, "null argument");
  if (b < 0 || b >= h->sp.B) return fail(MHPC_ERR_INVALID, "problem out of range");
  *desc = h->pl[b].desc;
  desc->vel_cmd = h->cmd[2 * (size_t)b];
  desc->height_cmd = h->cmd[2 * (size_t)b + 1];
  return MHPC_OK;
}

// Per-problem user commands (the batch axis over MHPCUserParameters::usrcmd).  New values reach
// the references at the next mhpc_initialize / mhpc_update_problem(s); until then an
// initialised handle refuses to solve (the ledger's command marks).
int api_set_commands(Handle* h, const double* vel, const double* height) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  const size_t B = h->sp.B;
  for (size_t b = 0; b < B; ++b)
    if ((vel && !std::isfinite(vel[b])) || (height && !std::isfinite(height[b])))
      return fail(MHPC_ERR_INVALID, "commands must be finite");
  std::vector<double> nc = h->cmd;
  for (size_t b = 0; b < B; ++b) {
    if (vel) nc[2 * b] = vel[b];
    if (height) nc[2 * b + 1] = height[b];
  }
  if (nc == h->cmd) return MHPC_OK;  // nothing changes: nothing pending
  HIPCHK(hipSetDevice(h->device));
  std::vector<Cmd> hc(B);
  for (size_t b = 0; b < B; ++b) hc[b] = Cmd{(real)nc[2 * b], (real)nc[2 * b + 1]};
  HIPCHK(hipMemcpyAsync(h->own.cmd.get(), hc.data(), B * sizeof(Cmd), hipMemcpyHostToDevice, h->main.s1));
  HIPCHK(hipStreamSynchronize(h->main.s1));
  if (h->initialized) {  // the problems whose value changed: pending until their next references
    for (size_t b = 0; b < B; ++b)
      if (nc[2 * b] != h->cmd[2 * b] || nc[2 * b + 1] != h->cmd[2 * b + 1]) h->led.command_changed((int)b);
  }
  h->cmd = nc;
  return MHPC_OK;
}
int api_get_commands(Handle* h, double* vel, double* height) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  for (size_t b = 0; b < (size_t)h->sp.B; ++b) {
    if (vel) vel[b] = h->cmd[2 * b];
    if (height) height[b] = h->cmd[2 * b + 1];
  }
  return MHPC_OK;
}

// The tracking reference x of one phase over a problem range, [count][N][xsize] (the cost
// kernels' own reference helpers, k_export_ref, through the export staging buffer).
int api_get_reference(Handle* h, int phase, int first, int count, double* xref) {
  if (!h || !xref) return fail(MHPC_ERR_INVALID, "null argument");
  if (!h->initialized) return fail(MHPC_ERR_STATE, "not initialized");
  int n = 0, N = 0;
  int rc = range_phase_shape(h, phase, first, count, &n, &N);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(launch_export_ref(h->sp, h->d, first, count, h->main.s1));
  std::vector<real> buf;
  auto ko = [&](int b) { return h->plan.lays[h->plan.lid[b]].ko[phase]; };
  return for_runs(first, count, ko, [&](int r0, int nb) -> int {
    if (int rc = copy_rows(h, h->d.out, KS, ko(r0), N, r0, nb, buf)) return rc;
    double* o = xref + (size_t)(r0 - first) * N * n;
    for (size_t i = 0; i < (size_t)nb * N; ++i)
      for (int j = 0; j < n; ++j) o[i * n + j] = buf[i * KS + j];
    return MHPC_OK;
  });
}

int api_num_layouts(Handle* h, int* n) {
  if (!h || !n) return fail(MHPC_ERR_INVALID, "null argument");
  *n = h->plan.nlay;  // (sp.ngrp counts (layout, parameter set) pairs)
  return MHPC_OK;
}

// the row length of get_scalars' V_phase / dV_phase (plan_groups: pmax)
int api_max_phases(Handle* h, int* n) {
  if (!h || !n) return fail(MHPC_ERR_INVALID, "null argument");
  *n = h->sp.pmax;
  return MHPC_OK;
}

int api_batch(Handle* h) { return h ? h->sp.B : 0; }

int api_get_desc(Handle* h, mhpc_problem_desc* desc) {
  if (!h || !desc) return fail(MHPC_ERR_INVALID, "null argument");
  return api_get_problem_desc(h, 0, desc);
}

int api_get_counters(Handle* h, mhpc_counters* c) {
  if (!h || !c) return fail(MHPC_ERR_INVALID, "null argument");
  memset(c, 0, sizeof *c);
  c->ddp_iters = (int64_t)h->cnt[C_DDP];
  c->bws_sweeps = (int64_t)h->cnt[C_BWS];
  c->bws_knots = (int64_t)h->cnt[C_BWS_KNOTS];
  c->ls_rollouts = (int64_t)h->cnt[C_LS];
  c->fwd_sweeps = (int64_t)h->cnt[C_FWD];
  c->partial_sweeps = (int64_t)h->cnt[C_PAR];
  c->solve_ms = h->solve_ms;
  return MHPC_OK;
}

int api_set_profiling(Handle* h, int on) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  h->profile = on != 0;
  return MHPC_OK;
}

int api_get_kernel_stats(Handle* h, double* ms, int64_t* launches,
                                     double* alg_bytes) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  for (int k = 0; k < NKERN; ++k) {
    if (ms) ms[k] = h->kms[k];
    if (launches) launches[k] = h->klaunch[k];
    if (alg_bytes) alg_bytes[k] = h->kbytes[k];
  }
  return MHPC_OK;
}

int api_set_kernel_variant(Handle* h, int which, int variant) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  SolveParams& sp = h->sp;
  if (which == MHPC_VARIANT_BWS) {
    if (variant < 0 || variant > MHPC_VARIANT_BWS_PAIRS2) return fail(MHPC_ERR_INVALID, "no such backward-sweep variant");
    sp.var_bws = variant;
    return MHPC_OK;
  }
  if (which == MHPC_VARIANT_OVERLAP) {
    if (variant < 0 || variant > MHPC_VARIANT_OVERLAP_OFF) return fail(MHPC_ERR_INVALID, "no such overlap variant");
    sp.var_overlap = variant;
    return MHPC_OK;
  }
  if (which == MHPC_VARIANT_RO_STORE) {
    if (variant < 0 || variant > MAXC) return fail(MHPC_ERR_INVALID, "stored trials must be 0..32");
    h->ro_store_req = variant;
    sp.ro_store = variant ? variant : ro_store_auto(sp);
    return MHPC_OK;
  }
  if (which == MHPC_VARIANT_SWEEP_BITS) {
    if (variant != 0 && variant != 64 && !(variant == 32 && sizeof(real) == 4))
      return fail(MHPC_ERR_INVALID, "sweep arithmetic must be 0 / 64 (double), or 32 (float) in an fp32 handle");
    h->sweep_bits = variant;
    return MHPC_OK;
  }
  if (which == MHPC_VARIANT_SNAP_ROUND) {
    if (variant < 0) return fail(MHPC_ERR_INVALID, "the snapshot round must be >= 1 problem, or 0");
    h->snap_round_req = variant;
    return MHPC_OK;
  }
  if (which == MHPC_VARIANT_SUBBATCH) {
    if (variant < 0 || variant > MHPC_MAX_SUBBATCH) return fail(MHPC_ERR_INVALID, "sub-batch count must be 0..4");
    h->nsub_req = variant;
    return MHPC_OK;
  }
  if (which != MHPC_VARIANT_RO) return fail(MHPC_ERR_INVALID, "no such kernel");
  if (variant < 0 || variant > MHPC_VARIANT_RO_FUSED) return fail(MHPC_ERR_INVALID, "no such line-search variant");
  const bool staged = variant == MHPC_VARIANT_RO_PAIR || variant == MHPC_VARIANT_RO_PIPE_STAGED ||
                      variant == MHPC_VARIANT_RO_FUSED_STAGED;
  if (staged && 64 / sp.n_cand > 6)  // ST_PPW problems per staged wave (mhpc_kernels.hip)
    return fail(MHPC_ERR_INVALID, "staged line-search variants need >= 10 candidates");
  if (variant == MHPC_VARIANT_RO_PAIR && 32 / sp.n_cand < 1)
    return fail(MHPC_ERR_INVALID, "the pair variant needs <= 32 candidates");
  sp.var_ro = variant;
  return MHPC_OK;
}

int api_get_kernel_flops(Handle* h, double* flops) {
  if (!h || !flops) return fail(MHPC_ERR_INVALID, "null argument");
  for (int k = 0; k < NKERN; ++k) flops[k] = h->kflops[k];
  return MHPC_OK;
}

int api_reset_kernel_stats(Handle* h) {
  if (!h) return fail(MHPC_ERR_INVALID, "null handle");
  for (int k = 0; k < NKERN; ++k) {
    h->kms[k] = 0; h->kbytes[k] = 0; h->kflops[k] = 0; h->klaunch[k] = 0;
  }
  return MHPC_OK;
}

void api_destroy(Handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // every stream of the handle drains before its buffers go (an error inside a solve can
  // leave work queued on the partials' or a sub-batch's streams)
  (void)sync_streams(h);
  delete h;
}

// ---- batched model evaluation hooks ---------------------------------------------------------
// Kernel-level parity hooks of this build's arithmetic type: mhpc_eval_* in the fp64 build,
// mhpc_eval_*_f32 in the fp32 one (the same signatures and output shapes; host arrays double,
// converted to real on the way in and back on the way out).
#ifdef MHPC_FP32
#define HOOK(name) name##_f32
#else
#define HOOK(name) name
#endif
#define HOOK_STR2(x) #x
#define HOOK_STR(x) HOOK_STR2(x)
#define HOOK_NAME(name) HOOK_STR(HOOK(name))
// the launch between the hook's inputs and its outputs' way back; fn: the exported name
#define HOOK_RUN(t, fn, launch)                                \
  do {                                                         \
    if (t.e == hipSuccess) t.e = (launch);                     \
    if (t.fetch() != hipSuccess) return dev_fail(fn, t.e);     \
    return MHPC_OK;                                            \
  } while (0)

// Whole-body dynamics, single-lane (pair = 0: xdot [n][14], y [n][4]) or lane pair (pair = 1:
// xdot [n][2][14], y [n][2][4])
static int eval_wb_dynamics(const char* fn, int device, int n, int mode, int pair, const double* x,
                            const double* u, double* xdot, double* y) {
  if (n < 1 || !x || !u || !xdot || !y || mode < 1 || mode > 4 || (pair != 0 && pair != 1))
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t L = pair ? 2 : 1;
  DevTemp<real> t;
  real *dx = t.in(x, (size_t)n * 14), *du = t.in(u, (size_t)n * 4);
  real *dxd = t.out(xdot, n * 14 * L), *dy = t.out(y, n * 4 * L);
  HOOK_RUN(t, fn,
           pair ? launch_eval_wb_dyn_pair(n, mode, dx, du, dxd, dy, nullptr)
                : launch_eval_wb_dyn(n, mode, dx, du, dxd, dy, nullptr));
}
#ifdef MHPC_FP32
extern "C" int mhpc_eval_wb_dynamics_f32(int device, int n, int mode, int pair, const double* x,
                                         const double* u, double* xdot, double* y) {
  return eval_wb_dynamics("mhpc_eval_wb_dynamics_f32", device, n, mode, pair, x, u, xdot, y);
}
#else
extern "C" int mhpc_eval_wb_dynamics(int device, int n, int mode, const double* x, const double* u,
                                     double* xdot, double* y) {
  return eval_wb_dynamics("mhpc_eval_wb_dynamics", device, n, mode, 0, x, u, xdot, y);
}
extern "C" int mhpc_eval_wb_dynamics_pair(int device, int n, int mode, const double* x,
                                          const double* u, double* xdot, double* y) {
  return eval_wb_dynamics("mhpc_eval_wb_dynamics_pair", device, n, mode, 1, x, u, xdot, y);
}
#endif

extern "C" int HOOK(mhpc_eval_wb_touchdown)(int device, int n, int foot, const double* x, double* h,
                                            double* hx, double* hxx, double* J, double* Jd) {
  if (n < 1 || !x || !h || !hx || !hxx || !J || !Jd || (foot != 0 && foot != 1))
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t m = n;
  DevTemp<real> t;
  real *dx = t.in(x, m * 14), *dh = t.out(h, m * 2), *dhx = t.out(hx, m * 14);
  real *dhxx = t.out(hxx, m * 196), *dJ = t.out(J, m * 14), *dJd = t.out(Jd, m * 14);
  HOOK_RUN(t, HOOK_NAME(mhpc_eval_wb_touchdown),
           launch_eval_wb_aux(n, foot, dx, dh, dhx, dhxx, dJ, dJd, nullptr));
}

extern "C" int HOOK(mhpc_eval_wb_partials)(int device, int n, int mode, const double* x,
                                           const double* u, double* Ac, double* Bc, double* C,
                                           double* D) {
  if (n < 1 || !x || !u || !Ac || !Bc || !C || !D || mode < 1 || mode > 4)
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t m = n;
  DevTemp<real> t;
  real *dx = t.in(x, m * 14), *du = t.in(u, m * 4), *dA = t.out(Ac, m * 196);
  real *dB = t.out(Bc, m * 56), *dC = t.out(C, m * 56), *dD = t.out(D, m * 16);
  HOOK_RUN(t, HOOK_NAME(mhpc_eval_wb_partials),
           launch_eval_wb_par(n, mode, dx, du, dA, dB, dC, dD, nullptr));
}

extern "C" int HOOK(mhpc_eval_wb_impact)(int device, int n, int foot, const double* x,
                                         double* xplus, double* Px) {
  if (n < 1 || !x || !xplus || !Px || (foot != 0 && foot != 1))
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t m = n;
  DevTemp<real> t;
  real *dx = t.in(x, m * 14), *dxp = t.out(xplus, m * 14), *dP = t.out(Px, m * 196);
  HOOK_RUN(t, HOOK_NAME(mhpc_eval_wb_impact),
           launch_eval_wb_impact(n, foot, dx, dxp, dP, nullptr));
}

extern "C" int HOOK(mhpc_eval_srb)(int device, int n, const double* x, const double* u,
                                   const double* foothold, const double* contact, double* xdot,
                                   double* Ac, double* Bc) {
  if (n < 1 || !x || !u || !foothold || !contact || !xdot || !Ac || !Bc)
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t m = n;
  DevTemp<real> t;
  real *dx = t.in(x, m * 6), *du = t.in(u, m * 4), *dp = t.in(foothold, m * 4);
  real *dc = t.in(contact, m * 2), *dxd = t.out(xdot, m * 6), *dA = t.out(Ac, m * 36);
  real* dB = t.out(Bc, m * 24);
  HOOK_RUN(t, HOOK_NAME(mhpc_eval_srb), launch_eval_srb(n, dx, du, dp, dc, dxd, dA, dB, nullptr));
}

// One elementary function at n points (MHPC_PRIM_*, include/mhpc_capi.h).
extern "C" int HOOK(mhpc_eval_primitive)(int device, int fn, int n, const double* a,
                                         const double* b, double* out) {
  const bool two = fn == MHPC_PRIM_REDUCED_BARRIER || fn == MHPC_PRIM_DIV_CONST;
  bool known = fn >= MHPC_PRIM_SINCOS && fn <= MHPC_PRIM_DIV_CONST;
#ifndef MHPC_FP32
  known = known && fn != MHPC_PRIM_SWEEP_RECIP_F32;
#endif
  if (n < 1 || !a || !out || !known || (two && !b) || n % eval_prim_group(fn))
    return fail(MHPC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(device));
  const size_t m = n;
  if (fn == MHPC_PRIM_SWEEP_RECIP) {  // the sweep's type, not the library's
    DevTemp<double> t;
    double *da = t.in(a, m), *dout = t.out(out, m);
    HOOK_RUN(t, HOOK_NAME(mhpc_eval_primitive), launch_eval_recip(n, da, dout, nullptr));
  }
  DevTemp<real> t;
#ifdef MHPC_FP32
  if (fn == MHPC_PRIM_SWEEP_RECIP_F32) {
    real *da = t.in(a, m), *dout = t.out(out, m);
    HOOK_RUN(t, HOOK_NAME(mhpc_eval_primitive), fsweep::launch_eval_recip(n, da, dout, nullptr));
  }
#endif
  const size_t w = fn <= MHPC_PRIM_SINCOS_N3_VK ? 2 : fn == MHPC_PRIM_REDUCED_BARRIER ? 3 : 1;
  real *da = t.in(a, m), *db = two ? t.in(b, m) : nullptr, *dout = t.out(out, m * w);
  HOOK_RUN(t, HOOK_NAME(mhpc_eval_primitive), launch_eval_prim(fn, n, da, db, dout, nullptr));
}

}  // namespace MHPC_NS
