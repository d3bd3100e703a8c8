// The host-side plan of a batch: per-problem layouts and parameter sets -> the groups the kernels
// run over.  Everything a per-problem change (layouts, gait steps, parameter sets, resets, copies)
// has to decide before it touches the device is here, as plain C++ with no HIP call and no
// handle: the descriptor checks, the gait step of one problem, the checks that a layout fits the
// arrays as they are, the merge of equal parameter sets, and plan_groups, which turns
// (layout, set) of every problem into a GroupPlan.  The runtime (mhpc_runtime.cpp) validates,
// plans, and only then commits a plan to the handle and the device (commit_groups); the host check
// (tests/native/plan_hostcheck.cpp) compiles this header with plain g++.  Option sets are no part of
// the grouping: their checks, the table of records (plan_options), the iteration caps of a scope
// (scope_caps) and the launch schedule those give (solve_ops) are here as well
// (tests/native/option_hostcheck.cpp).  So is what every call on some problems of a live batch
// shares (tests/native/ledger_hostcheck.cpp): the checked problem list (ProblemList), the packer of
// caller rows into device rows (pack_rows), the scope of a list (solve_scope: tick and reset), and
// the per-problem call-order state with its transitions (Ledger).
//
// A function that can refuse returns MHPC_ERR_INVALID and sets *msg (a literal); it changes
// nothing it was given unless its comment says otherwise.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "mhpc_solver.h"

namespace MHPC_NS {

// Per-problem phase layout: the descriptor (gait point) and the phase-buffer rotation of the
// receding-horizon loop (MHPCLocomotion::update_problem rotates pidx_WB / pidx_FB by one per
// call, MHPCLocomotion.cpp:111-121: after r calls phase i uses buffer (i + r) mod n).
struct ProbLayout {
  mhpc_problem_desc desc;
  int rot_wb, rot_fb;
};
// Algorithmic bytes per problem of one layout
struct ByteModel {
  double roll_read = 0, roll_write = 0, roll_term = 0, par = 0, init = 0, cost = 0;
  double roll_flops = 0;  // one trial rollout (the line search's flop model)
};

inline int plan_refuse(const char** msg, const char* text) {
  if (msg) *msg = text;
  return MHPC_ERR_INVALID;
}

// ---- descriptors ----------------------------------------------------------------------------
inline int check_desc(const mhpc_problem_desc* d, const char** msg) {
  if (!d) return plan_refuse(msg, "null descriptor");
  const int P = d->n_wb + d->n_fb;
  if (d->n_wb < 0 || d->n_fb < 0 || P < 1 || P > MHPC_MAX_PHASES)
    return plan_refuse(msg, "phase count out of range");
  if (d->precision != 64 && d->precision != 32) return plan_refuse(msg, "precision must be 64 or 32");
  int NK = 0;
  for (int p = 0; p < P; ++p) {
    if (d->mode_seq[p] < 1 || d->mode_seq[p] > 4) return plan_refuse(msg, "mode out of range");
    if (d->N[p] < 2) return plan_refuse(msg, "each phase needs N >= 2");
    NK += d->N[p];
  }
  if (NK > MHPC_MAX_KNOTS) return plan_refuse(msg, "too many knots");
  if (!(d->dt_wb > 0) || !(d->dt_fb > 0)) return plan_refuse(msg, "dt must be positive");
  return MHPC_OK;
}
// A descriptor given for some problems of a live handle (mhpc_set_layouts, mhpc_reset_problems):
// valid, and with the precision and the command of the handle's own descriptor.
inline int check_layout_desc(const mhpc_problem_desc& d, const mhpc_problem_desc& handle_desc,
                             const char** msg) {
  if (int rc = check_desc(&d, msg)) return rc;
  if (d.precision != handle_desc.precision)
    return plan_refuse(msg, "a layout's precision differs from the handle's");
  if (d.vel_cmd != handle_desc.vel_cmd || d.height_cmd != handle_desc.height_cmd)
    return plan_refuse(msg, "a layout's vel_cmd / height_cmd differs from the handle's");
  return MHPC_OK;
}

// A descriptor normalised for comparison (entries past its phases and reserved fields zero)
inline mhpc_problem_desc norm_desc(const mhpc_problem_desc& in) {
  mhpc_problem_desc d;
  memset(&d, 0, sizeof d);
  d.n_wb = in.n_wb;
  d.n_fb = in.n_fb;
  for (int p = 0; p < in.n_wb + in.n_fb; ++p) {
    d.mode_seq[p] = in.mode_seq[p];
    d.N[p] = in.N[p];
  }
  d.dt_wb = in.dt_wb;
  d.dt_fb = in.dt_fb;
  d.vel_cmd = in.vel_cmd;
  d.height_cmd = in.height_cmd;
  d.precision = in.precision;
  return d;
}

// Phase layout of a descriptor: modes, knot counts and offsets, partials work items, and the
// phase buffers after rot_wb / rot_fb rotations (MHPCLocomotion::update_problem).
inline void build_layout(Layout& L, const mhpc_problem_desc& desc, int rot_wb, int rot_fb) {
  memset(&L, 0, sizeof L);
  L.P = desc.n_wb + desc.n_fb;
  L.n_wb = desc.n_wb;
  int ko = 0, items = 0, items_v = 0;
  for (int p = 0; p < L.P; ++p) {
    const bool wb = p < desc.n_wb;
    L.mode[p] = desc.mode_seq[p];
    L.N[p] = desc.N[p];
    L.ko[p] = ko;
    L.xs[p] = wb ? 14 : 6;
    L.dt[p] = wb ? desc.dt_wb : desc.dt_fb;
    L.buf[p] = wb ? (p + rot_wb) % desc.n_wb : desc.n_wb + (p - desc.n_wb + rot_fb) % desc.n_fb;
    ko += desc.N[p];
    L.par_knot_off[p] = items;
    L.par_imp_off[p] = items_v;
    if (wb) {
      items += desc.N[p] - 1;
      items_v += (L.mode[p] == 2 || L.mode[p] == 4) ? 14 : 0;
    }
  }
  for (int p = L.P; p <= MAXP; ++p) {
    L.par_knot_off[p] = items;
    L.par_imp_off[p] = items_v;
  }
  L.par_knots = items;
  L.par_imp = items_v;
  L.NK = ko;
}

// ---- the byte model -------------------------------------------------------------------------
// Algorithmic HBM bytes of one problem for each kernel's unit of work.
constexpr double kB = sizeof(real);  // bytes per element of the solve's arithmetic type

// Line-search flop model per trial knot (SURVEY.md 8d secondary roofline): the reference's
// dynamics in CasADi's generated-code assignment counts (Dyn_BS / Dyn_FS 2301,
// Dyn_FL 1441, FBDynamics 44 -- scalar operations incl. loads, so an upper estimate), plus the
// feedback u = u_nom + eps du + K (x - x_nom) and the Euler step (WB: 14 + 4 * 28 + 8 + 28;
// SRB: 6 + 4 * 12 + 8 + 12).  The running costs (the second wave) are not counted.
inline double ro_knot_flops(int mode, bool wb) {
  if (!wb) return 44 + 74;
  return (mode == 1 || mode == 3 ? 2301.0 : 1441.0) + 162;
}

inline ByteModel byte_model(const Layout& L) {
  ByteModel m;
  double rr = 14 * 8, rw = 0, rt = 0, pb = 0, ib = L.NK * kB, cb = 0;
  for (int p = 0; p < L.P; ++p) {
    const bool wb = p < L.n_wb;
    const int n = wb ? 14 : 6, N = L.N[p];
    // nominal x,u (n+4) + K (4n) + du (4) read once per problem (the candidates of a
    // problem share them)
    rr += (N - 1) * kB * ((n + 4) + 4 * n + 4);
    // a storing candidate writes x,u,y of every knot, every candidate x at the last knot
    rw += (N - 1) * kB * (n + 8);
    rt += n * kB;
    m.roll_flops += (N - 1) * ro_knot_flops(L.mode[p], wb);
    // k_cost: nominal x,u(,y) of every knot + refpos
    cb += (N - 1) * kB * (n + 4 + (wb ? 4 : 0) + 1) + kB * (n + 1);
    // k_init: x,u,y written for every knot (WB and SRB)
    if (!wb) ib += N * kB * 14;
    if (wb) {
      const bool imp = L.mode[p] == 2 || L.mode[p] == 4;
      // x,u read; the record written without its four zero columns (written once at create)
      pb += (N - 1) * kB * (18 + PS - 4 * 9) + (imp ? kB * (14 + 196) : 0.0);
      ib += N * kB * 22;
    }
  }
  m.roll_read = rr;
  m.roll_write = rw;
  m.roll_term = rt;
  m.par = pb;
  m.init = ib;
  m.cost = cb;
  return m;
}

// ---- parameter sets -------------------------------------------------------------------------
// Parameter sets compare by value, entry by entry (CostParams holds nothing but reals).
inline bool same_params(const CostParams& a, const CostParams& b) {
  const real *x = (const real*)&a, *y = (const real*)&b;
  for (size_t i = 0; i < sizeof(CostParams) / sizeof(real); ++i)
    if (!(x[i] == y[i])) return false;
  return true;
}
// Merge the sets that compare equal and drop the ones no problem uses (first occurrence
// kept, order preserved); `of` is renumbered accordingly.
inline void merge_sets(std::vector<CostParams>& sets, std::vector<int>& of) {
  std::vector<int> to(sets.size(), -1);
  std::vector<char> used(sets.size(), 0);
  for (int s : of) used[s] = 1;
  std::vector<CostParams> out;
  for (size_t i = 0; i < sets.size(); ++i) {
    if (!used[i]) continue;
    for (size_t j = 0; j < out.size() && to[i] < 0; ++j)
      if (same_params(out[j], sets[i])) to[i] = (int)j;
    if (to[i] < 0) {
      to[i] = (int)out.size();
      out.push_back(sets[i]);
    }
  }
  for (int& s : of) s = to[s];
  sets.swap(out);
}

// ---- option sets ----------------------------------------------------------------------------
// Integer iteration cap of a (double) max_AL_iter / max_DDP_iter: the last i of the reference's
// `for (i = 1; i <= max_iter; ++i)` (MultiPhaseDDP.cpp:168, 192), 0 when the loop never runs
// (0, negative, a fraction below 1); a fraction above rounds down.  check_option bounds v.
constexpr double kMaxIterBudget = 1 << 20;
inline int option_cap(double v) {
  int cap = 0;
  for (int i = 1; i <= v && i <= (int)kMaxIterBudget; ++i) cap = i;
  return cap;
}
// Trials of the line-search grid 1, alpha, alpha^2, ... > 1e-10 exactly as
// MultiPhaseDDP::forward_iteration generates it (:130-151), into eps when given; more than max:
// max + 1 is returned.
inline int option_grid(double alpha, int max, real* eps) {
  int nc = 0;
  for (double e = 1; e > pow(0.1, 10); e *= alpha) {
    if (nc == max) return max + 1;
    if (eps) eps[nc] = (real)e;
    ++nc;
  }
  return nc;
}
// An option record as mhpc_create and the option setters take it: alpha in (0,1) with a grid of
// at most MAXC trials, every real field finite, iteration budgets no larger than kMaxIterBudget
// (a schedule of that length could not be issued anyway).  alpha_of != null (the setters): alpha
// must be, bit for bit, the handle's -- it fixes the line-search grid and with it the arrays' shape.
inline int check_option(const mhpc_hsddp_option* o, const double* alpha_of, const char** msg) {
  if (!o) return plan_refuse(msg, "null option");
  if (!(o->alpha > 0 && o->alpha < 1)) return plan_refuse(msg, "alpha must be in (0,1)");
  if (alpha_of && memcmp(&o->alpha, alpha_of, sizeof(double)) != 0)
    return plan_refuse(msg, "alpha differs from the handle's (it fixes the line-search grid)");
  if (option_grid(o->alpha, MAXC, nullptr) > MAXC)
    return plan_refuse(msg, "line search needs more than 32 trials (alpha too large)");
  const double f[] = {o->gamma,      o->update_penalty, o->update_relax, o->update_regularization,
                      o->update_ReB, o->max_DDP_iter,   o->max_AL_iter,  o->DDP_thresh,
                      o->AL_thresh};
  for (double v : f)
    if (!std::isfinite(v)) return plan_refuse(msg, "option fields must be finite");
  if (o->max_DDP_iter > kMaxIterBudget || o->max_AL_iter > kMaxIterBudget)
    return plan_refuse(msg, "iteration budget too large");
  return MHPC_OK;
}
// A record normalised for comparison and reporting (the reserved field zero); records compare
// bit for bit, every field.
inline mhpc_hsddp_option norm_option(const mhpc_hsddp_option& in) {
  mhpc_hsddp_option o = in;
  o.reserved = 0;
  return o;
}
inline bool same_option(const mhpc_hsddp_option& a, const mhpc_hsddp_option& b) {
  const mhpc_hsddp_option x = norm_option(a), y = norm_option(b);
  static_assert(sizeof(mhpc_hsddp_option) == 10 * sizeof(double) + 4 * sizeof(int32_t), "no padding");
  return memcmp(&x, &y, sizeof x) == 0;
}
// The record as the kernels read it (mhpc_solver.h, OptRec), with its iteration caps.
inline OptRec option_record(const mhpc_hsddp_option& o) {
  OptRec r;
  memset(&r, 0, sizeof r);
  r.gamma = (real)o.gamma;
  r.DDP_thresh = (real)o.DDP_thresh;
  r.AL_thresh = (real)o.AL_thresh;
  r.update_penalty = (real)o.update_penalty;
  r.update_relax = (real)o.update_relax;
  r.update_regularization = (real)o.update_regularization;
  r.update_ReB = (real)o.update_ReB;
  r.AL_active = o.AL_active ? 1 : 0;
  r.ReB_active = o.ReB_active ? 1 : 0;
  r.n_al = option_cap(o.max_AL_iter);
  r.max_ddp = option_cap(o.max_DDP_iter);
  return r;
}
// The option table of a handle: at most MAXO slots, each a record and the number of problems that
// use it (0: the slot is free -- unused records are dropped), and each problem's slot.  Slots are
// stable: a problem whose record does not change keeps its slot, so an assignment touches the
// device entries of the changed problems alone.  Equal records share a slot (merged).
struct OptTable {
  std::vector<mhpc_hsddp_option> rec;  // [slots] (a free slot keeps its last record)
  std::vector<int> use;                // [slots]
  std::vector<int> of;                 // [B] slot of each problem
  int in_use() const { return (int)std::count_if(use.begin(), use.end(), [](int u) { return u > 0; }); }
  int find(const mhpc_hsddp_option& o) const {  // the used slot holding o, -1 if none
    for (size_t s = 0; s < rec.size(); ++s)
      if (use[s] > 0 && same_option(rec[s], o)) return (int)s;
    return -1;
  }
};
// Problem b gets record want[b] (checked records): t becomes the new table, changed the problems
// whose record differs from the one they had, in problem order.  Refused, with t and changed as
// they were, when the distinct records in use would exceed MAXO.
inline int plan_options(OptTable& t, const std::vector<const mhpc_hsddp_option*>& want,
                        std::vector<int>& changed, const char** msg) {
  OptTable n = t;
  std::vector<int> ch;
  for (size_t b = 0; b < want.size(); ++b)
    if (!same_option(t.rec[t.of[b]], *want[b])) {
      ch.push_back((int)b);
      --n.use[n.of[b]];
    }
  for (int b : ch) {
    int s = n.find(*want[b]);
    for (size_t f = 0; s < 0 && f < n.rec.size(); ++f)
      if (n.use[f] == 0) s = (int)f;
    if (s < 0) {
      if ((int)n.rec.size() == MAXO)
        return plan_refuse(msg, "more than MHPC_MAX_OPTION_SETS distinct option sets");
      s = (int)n.rec.size();
      n.rec.push_back(norm_option(*want[b]));
      n.use.push_back(0);
    }
    if (n.use[s] == 0) n.rec[s] = norm_option(*want[b]);
    ++n.use[s];
    n.of[b] = s;
  }
  t = std::move(n);
  changed = std::move(ch);
  return MHPC_OK;
}

// ---- the solve schedule -----------------------------------------------------------------------
// The iteration caps a scope's schedule runs to: the largest n_al and max_ddp among its problems
// (list == nullptr: every problem, the whole batch).  A problem with smaller caps sits the rest
// out on the device (in_op, mhpc_device.h).
// min_*: the smallest caps, al_uniform: the problems' common AL_active (-1: they differ) -- what
// lets the schedule's kernels skip the per-problem reads (SolveParams::min_n_al ...).
struct ScopeCaps {
  int n_al = 0, max_ddp = 0;
  int min_n_al = 0, min_max_ddp = 0, al_uniform = -1;
};
inline ScopeCaps scope_caps(const OptTable& t, const int* list, int n) {
  std::vector<char> used(t.rec.size(), 0);
  if (list)
    for (int i = 0; i < n; ++i) used[t.of[list[i]]] = 1;
  else
    for (int s : t.of) used[s] = 1;
  ScopeCaps c;
  bool first = true;
  for (size_t s = 0; s < t.rec.size(); ++s) {
    if (!used[s]) continue;
    const int a = option_cap(t.rec[s].max_AL_iter), dd = option_cap(t.rec[s].max_DDP_iter);
    const int on = t.rec[s].AL_active ? 1 : 0;
    c.n_al = std::max(c.n_al, a);
    c.max_ddp = std::max(c.max_ddp, dd);
    c.min_n_al = first ? a : std::min(c.min_n_al, a);
    c.min_max_ddp = first ? dd : std::min(c.min_max_ddp, dd);
    c.al_uniform = first ? on : (c.al_uniform == on ? on : -1);
    first = false;
  }
  return c;
}
// MultiPhaseDDP::solve (MultiPhaseDDP.cpp:154-289) as a list of launches for iteration caps
// (n_al, max_ddp); full: the first forward_sweep(0) is a real rollout.  al / ddp name the
// iteration an op belongs to (OP_AL: the AL iteration it closes, 1 for the lone update of a
// schedule without AL iterations), last marks the schedule's final op.
enum { OP_COST, OP_FULL, OP_PAR, OP_BWS, OP_LS, OP_AL };
struct SolveOp {
  int kind, al, ddp, last;
};
inline std::vector<SolveOp> solve_ops(ScopeCaps c, bool full) {
  std::vector<SolveOp> ops;
  for (int al = 1; al <= c.n_al; ++al) {
    // forward_sweep(0); a real rollout for the rotated nominal of update_problem
    ops.push_back({al == 1 && full ? OP_FULL : OP_COST, al, 0, 0});
    ops.push_back({OP_PAR, al, 0, 0});
    for (int ddp = 1; ddp <= c.max_ddp; ++ddp) {
      ops.push_back({OP_BWS, al, ddp, 0});
      ops.push_back({OP_LS, al, ddp, 0});  // forward_iteration
      if (ddp < c.max_ddp) ops.push_back({OP_PAR, al, ddp, 0});
    }
    ops.push_back({OP_AL, al, 0, al == c.n_al ? 1 : 0});
  }
  if (c.n_al == 0) ops.push_back({OP_AL, 1, 0, 1});
  return ops;
}

// ---- a layout against the arrays as they are (mhpc_reset_problems, mhpc_copy_problems) --------
// Neither call re-strides or reallocates: the layout must fit the knot stride NK and, when the
// phase-buffer store is live (store_valid), its buffers of nbk knots and its spmax buffers a
// problem.  copy: the wording of mhpc_copy_problems, whose arrays are the destination's.
inline int fits_arrays(const ProbLayout& q, int NK, bool store_valid, int nbk, int spmax, bool copy,
                       const char** msg) {
  const int P = q.desc.n_wb + q.desc.n_fb;
  int nk = 0;
  for (int p = 0; p < P; ++p) {
    nk += q.desc.N[p];
    if (store_valid && q.desc.N[p] > nbk)
      return plan_refuse(msg, copy ? "phase longer than the destination's phase buffers"
                                   : "phase longer than the phase buffers");
  }
  if (nk > NK)
    return plan_refuse(
        msg, copy ? "source layout longer than the destination's knot stride (a copy never grows the arrays)"
                  : "layout longer than the knot stride (a reset never grows the arrays)");
  if (store_valid && P > spmax)
    return plan_refuse(msg, copy ? "more phases than the destination's phase-buffer store holds"
                                 : "more phases than the phase-buffer store holds");
  return MHPC_OK;
}
// Width of the caller's x0 rows: 14 once any problem has a whole-body phase, else 6.  (Of layouts
// not planned yet; x0_row_of(GroupPlan) below answers for an installed plan from its groups.)
inline int x0_row_of(const std::vector<ProbLayout>& pl) {
  for (const ProbLayout& q : pl)
    if (q.desc.n_wb > 0) return 14;
  return 6;
}

// ---- a list of problems (mhpc_tick_problems, mhpc_reset_problems, mhpc_copy_problems) ----------
// n problems of a batch of B, each in range and none twice; at[b] is problem b's place in the list
// (-1: not listed).  copy: the wording of mhpc_copy_problems, whose list is the destinations.
// Entry by entry (begin, then add for each in turn), so a caller with more to check per entry
// keeps the order of its refusals.
struct ProblemList {
  std::vector<int> at;
  int n = 0;  // entries added
  bool copy = false;
  int begin(int count, int B, bool copy_wording, const char** msg) {
    copy = copy_wording;
    if (count < 1 || count > B)
      return plan_refuse(msg, copy ? "n must be 1..batch of the destination" : "n must be 1..batch");
    at.assign(B, -1);
    n = 0;
    return MHPC_OK;
  }
  int add(int b, const char** msg) {
    if (b < 0 || b >= (int)at.size()) return plan_refuse(msg, "problem out of range");
    if (at[b] >= 0)
      return plan_refuse(msg, copy ? "destination problem listed twice" : "problem listed twice");
    at[b] = n++;
    return MHPC_OK;
  }
};

// ---- one problem's gait steps (mhpc_update_problems) ------------------------------------------
// MHPCLocomotion::update_problem's host part, `steps` times: advance the gait by one mode, recompute
// mode sequence and knot counts (Gait::get_next_mode / get_mode_seq / get_timings, Gait.h:48-77),
// rotate the WB and SRB phase buffers by one.  nbk: knots of a phase buffer.  q and cmode are the
// caller's working copies: a refusal leaves them partly advanced.
inline int advance_gait(ProbLayout& q, int& cmode, const mhpc_gait& gait, int steps, int nbk,
                        const char** msg) {
  auto next_mode = [&](int m) {
    for (int i = 0; i < gait.n_modes; ++i)
      if (gait.modes[i] == m) return gait.modes[(i + 1) % gait.n_modes];
    return -1;  // the reference falls off the end of a non-void function here
  };
  mhpc_problem_desc& nd = q.desc;
  const int P = nd.n_wb + nd.n_fb;
  for (int step = 0; step < steps; ++step) {
    const int cm = next_mode(cmode);
    if (cm < 0) return plan_refuse(msg, "current mode is not in the gait");
    cmode = cm;
    nd.mode_seq[0] = cm;
    for (int p = 1; p < P; ++p) nd.mode_seq[p] = next_mode(nd.mode_seq[p - 1]);
    int NK = 0;
    for (int p = 0; p < P; ++p) {
      const float tm = gait.timings[nd.mode_seq[p] - 1];
      const double dt = p < nd.n_wb ? nd.dt_wb : nd.dt_fb;
      nd.N[p] = (int)round((double)tm / dt);  // round(float timing / (double) dt)
      if (nd.N[p] < 2) return plan_refuse(msg, "gait timing gives a phase with N < 2");
      if (nd.N[p] > nbk) return plan_refuse(msg, "phase longer than the phase buffers");
      NK += nd.N[p];
    }
    if (NK > MHPC_MAX_KNOTS) return plan_refuse(msg, "too many knots");
    // pidx_WB / pidx_FB: front -> back (MHPCLocomotion.cpp:111-121); kept reduced, so a
    // long receding-horizon loop never overflows the count
    q.rot_wb = (q.rot_wb + 1) % std::max(nd.n_wb, 1);
    q.rot_fb = (q.rot_fb + 1) % std::max(nd.n_fb, 1);
  }
  return MHPC_OK;
}

// ---- groups ---------------------------------------------------------------------------------
// The groups of a batch: the distinct (layout, set) pairs in use, where a layout is a
// (descriptor, buffer rotation) pair; longest layout first (its blocks head every launch: the
// long blocks start first in a mixed batch), layouts of equal length in the order of their first
// problem, then by set, the problems of each group in batch order.  Group g has its own Layout
// record (a layout that several sets share is stored once per group, so lays[lid[b]] stays
// problem b's layout).
struct GroupPlan {
  std::vector<Layout> lays;              // [ngrp] each group's layout
  std::vector<mhpc_problem_desc> ldesc;  // [ngrp] its normalised descriptor
  std::vector<ByteModel> bym;            // [ngrp] its byte model
  std::vector<int> gset;                 // [ngrp] each group's parameter set
  std::vector<int> lid, gidx;            // [B] each problem's group; the problems grouped
  int nlay = 0;                          // distinct layouts (ngrp counts (layout, set) pairs)
  int NK = 0;                            // knots of the longest layout
  // the grouping's fields of SolveParams, under their names there
  int ngrp = 0, ident = 1, pmax = 0, split_ok = 0, stage_fits = 1;
  int go[MAXL + 1] = {}, gpk[MAXL] = {}, gpi[MAXL] = {};

  void to_params(SolveParams& sp) const {  // (sp.NK is the arrays' stride: not the plan's to set)
    sp.ngrp = ngrp;
    sp.ident = ident;
    sp.pmax = pmax;
    sp.split_ok = split_ok;
    sp.stage_fits = stage_fits;
    std::copy(go, go + MAXL + 1, sp.go);
    std::copy(gpk, gpk + MAXL, sp.gpk);
    std::copy(gpi, gpi + MAXL, sp.gpi);
  }
};

// pl [B], pset_of [B] -> out.  Refused, with out as it was, for more than MAXL distinct layouts or
// more than MAXL (layout, set) pairs.
inline int plan_groups(const std::vector<ProbLayout>& pl, const std::vector<int>& pset_of,
                       GroupPlan& out, const char** msg) {
  const int B = (int)pl.size();
  std::map<std::string, int> seen;
  std::vector<ProbLayout> uniq;
  std::vector<int> first_lid(B);
  for (int b = 0; b < B; ++b) {
    ProbLayout k;
    memset(&k, 0, sizeof k);
    k.desc = norm_desc(pl[b].desc);
    k.rot_wb = k.desc.n_wb > 0 ? pl[b].rot_wb % k.desc.n_wb : 0;
    k.rot_fb = k.desc.n_fb > 0 ? pl[b].rot_fb % k.desc.n_fb : 0;
    const std::string key((const char*)&k, sizeof k);
    auto it = seen.find(key);
    if (it == seen.end()) {
      if ((int)uniq.size() == MAXL) return plan_refuse(msg, "more than MHPC_MAX_LAYOUTS distinct layouts");
      it = seen.emplace(key, (int)uniq.size()).first;
      uniq.push_back(k);
    }
    first_lid[b] = it->second;
  }
  const int L = (int)uniq.size();
  std::vector<Layout> lay(L);
  for (int l = 0; l < L; ++l) build_layout(lay[l], uniq[l].desc, uniq[l].rot_wb, uniq[l].rot_fb);
  std::vector<int> order(L), rank(L);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return lay[a].NK > lay[c].NK; });
  for (int l = 0; l < L; ++l) rank[order[l]] = l;
  // the (layout rank, set) pairs in use, in that order
  std::map<std::pair<int, int>, int> grp;
  for (int b = 0; b < B; ++b) grp[{rank[first_lid[b]], pset_of[b]}] = 0;
  const int G = (int)grp.size();
  if (G > MAXL)
    return plan_refuse(msg, "more than MHPC_MAX_LAYOUTS distinct (layout, parameter set) pairs");
  GroupPlan n;
  n.lays.resize(G);
  n.ldesc.resize(G);
  n.bym.resize(G);
  n.gset.resize(G);
  n.nlay = L;
  int ng = 0;
  for (auto& kv : grp) {
    const int g = kv.second = ng++;
    const Layout& Lg = lay[order[kv.first.first]];
    n.lays[g] = Lg;
    n.ldesc[g] = uniq[order[kv.first.first]].desc;
    n.bym[g] = byte_model(Lg);
    n.gset[g] = kv.first.second;
    n.NK = std::max(n.NK, Lg.NK);
    n.pmax = std::max(n.pmax, Lg.P);
    if (Lg.n_wb > 0 && Lg.P > Lg.n_wb) n.split_ok = 1;
    for (int p = 0; p < Lg.P; ++p)
      if (Lg.N[p] > ST_RMAX) n.stage_fits = 0;
    n.gpk[g] = Lg.par_knots;
    n.gpi[g] = Lg.par_imp;
  }
  n.lid.resize(B);
  std::vector<int> cnt(G + 1, 0);
  for (int b = 0; b < B; ++b) {
    n.lid[b] = grp[{rank[first_lid[b]], pset_of[b]}];
    ++cnt[n.lid[b] + 1];
  }
  n.ngrp = G;
  for (int g = 0; g < G; ++g) cnt[g + 1] += cnt[g];
  for (int g = 0; g <= G; ++g) n.go[g] = cnt[g];
  n.gidx.resize(B);
  for (int b = 0; b < B; ++b) {
    const int pos = cnt[n.lid[b]]++;
    n.gidx[pos] = b;
    if (pos != b) n.ident = 0;
  }
  out = std::move(n);
  return MHPC_OK;
}

// ---- the scope of a solve (mhpc_solve: the batch; mhpc_tick_problems, and mhpc_reset_problems for
// its init kernels: a list) ----------------------------------------------------------------------
// What the solve schedule runs over: `order`, the scope's problems by group, then problem number
// (the scope's gidx), and go[], each group's range of positions in it (a group with no problem in
// the scope is an empty range).  The scope of the whole batch is the plan's own gidx / go[].
// With fresh problems in a solve that starts with the real rollout, that first op runs as two
// launches over `split`: the rolled-out problems first, then the fresh ones (k_cost), each in the
// order of `order`, so a contiguous range of positions stays contiguous and grouped in both
// halves.  nf[pos] = problems before position pos that are not fresh (nf[n] = nnf, their total).
struct SolveScope {
  std::vector<int> order;
  int ngrp = 0;
  int go[MAXL + 1] = {};
  std::vector<int> split, nf;
  int nnf = 0;
  int size() const { return (int)order.size(); }
};
// plan: the installed plan; list: n distinct problems of it in any order; fresh: [B] flags by
// problem number (empty: none fresh).
inline SolveScope solve_scope(const GroupPlan& plan, const std::vector<int>& list,
                              const std::vector<char>& fresh) {
  SolveScope s;
  s.ngrp = plan.ngrp;
  s.order = list;
  std::sort(s.order.begin(), s.order.end(), [&](int a, int c) {
    return plan.lid[a] != plan.lid[c] ? plan.lid[a] < plan.lid[c] : a < c;
  });
  for (int b : s.order) ++s.go[plan.lid[b] + 1];
  for (int g = 0; g < plan.ngrp; ++g) s.go[g + 1] += s.go[g];
  const int n = s.size();
  s.nf.resize(n + 1);
  for (int pos = 0; pos < n; ++pos) {
    s.nf[pos] = s.nnf;
    s.nnf += !(!fresh.empty() && fresh[s.order[pos]]);
  }
  s.nf[n] = s.nnf;
  s.split.resize(n);
  for (int pos = 0; pos < n; ++pos) {
    const bool f = !fresh.empty() && fresh[s.order[pos]];
    s.split[f ? s.nnf + pos - s.nf[pos] : s.nf[pos]] = s.order[pos];
  }
  return s;
}
// A sub-batch's share of a scope: positions [b0, b1), each group's range clipped to them.
inline void scope_clip(const int* go, int ngrp, int b0, int b1, int* out) {
  for (int g = 0; g <= ngrp; ++g) out[g] = std::min(std::max(go[g], b0), b1);
}
// The two halves of ranges go[] (a scope's, or a sub-batch's clipped ones) as ranges of `split`:
// gof the rolled-out problems, goc the fresh ones.
inline void scope_split(const SolveScope& s, const int* go, int* gof, int* goc) {
  for (int g = 0; g <= s.ngrp; ++g) {
    gof[g] = s.nf[go[g]];
    goc[g] = s.nnf + go[g] - s.nf[go[g]];
  }
}

// ---- caller rows -> device rows ---------------------------------------------------------------
inline int x0_row_of(const GroupPlan& plan) {
  for (const Layout& L : plan.lays)
    if (L.n_wb > 0) return 14;
  return 6;
}
// Caller rows src [..][n_s][r] (r = x0_row_of(plan)) as `count` device rows of [n_s][14]: a problem
// with a whole-body phase has 14 entries, an SRB-only one the first 6 of its row (nothing past
// them is read); the rest is zero.  Destination row j is problem prob[j]'s (null: first + j) and
// comes from the caller's row at[that problem] (null: row j).
template <class E>
std::vector<E> pack_rows(const GroupPlan& plan, int count, int n_s, const double* src, int first,
                         const int32_t* prob = nullptr, const int* at = nullptr) {
  const size_t r = x0_row_of(plan), S = n_s;
  std::vector<E> out((size_t)count * S * 14, E(0));
  for (int j = 0; j < count; ++j) {
    const int b = prob ? prob[j] : first + j;
    const int nb = plan.lays[plan.lid[b]].n_wb > 0 ? 14 : 6;
    const double* from = src + (size_t)(at ? at[b] : j) * S * r;
    for (size_t t = 0; t < S; ++t)
      std::copy(from + t * r, from + t * r + nb, out.begin() + ((size_t)j * S + t) * 14);
  }
  return out;
}

// ---- per-problem call-order state ---------------------------------------------------------------
// What the runtime remembers per problem between calls, and the events that change it.
//  fresh: k_init wrote the problem's nominal since the last solve (mhpc_reset_problems) and no gait
//    step rotated it: in a solve that starts with the real rollout its first forward_sweep(0) is
//    still the cost evaluation, as after mhpc_initialize (the fp32 k_init rounds its warm start its
//    own way, so only k_cost continues it bit for bit).
//  open: mhpc_initialize / mhpc_reset_problems left the problem's SRB nominal zero because its
//    option record has no AL iteration (k_init_params), and no solve has covered it since.
//  mark: the problem's command changed since its references were last generated.
// The counts follow the flags here and nowhere else.
class Ledger {
  std::vector<char> fresh_, open_, mark_;
  int nfresh_ = 0, nmark_ = 0;
  static void set(std::vector<char>& f, int& count, int b, bool v) {
    count += (v ? 1 : 0) - (f[b] ? 1 : 0);
    f[b] = v;
  }
  static void fill(std::vector<char>& f, int& count, bool v) {
    std::fill(f.begin(), f.end(), v ? 1 : 0);
    count = v ? (int)f.size() : 0;
  }

 public:
  explicit Ledger(int B = 0) : fresh_(B, 0), open_(B, 0), mark_(B, 0) {}
  int size() const { return (int)fresh_.size(); }
  bool fresh(int b) const { return fresh_[b]; }
  bool open(int b) const { return open_[b]; }
  bool marked(int b) const { return mark_[b]; }
  int nfresh() const { return nfresh_; }
  int nmarked() const { return nmark_; }
  bool cmd_pending() const { return nmark_ > 0; }  // any command mark
  const std::vector<char>& fresh_flags() const { return fresh_; }  // (solve_scope)

  // mhpc_initialize: nobody fresh; no_al(b): problem b's record has no AL iteration
  template <class NoAl>
  void initialized(NoAl no_al) {
    fill(fresh_, nfresh_, false);
    for (int b = 0; b < size(); ++b) open_[b] = no_al(b);
  }
  // mhpc_solve: every problem solved, every later first sweep the real rollout
  void solved() {
    fill(fresh_, nfresh_, false);
    std::fill(open_.begin(), open_.end(), 0);
  }
  // mhpc_tick_problems: the listed problems have their references and their solve
  void ticked(int n, const int32_t* list) {
    for (int i = 0; i < n; ++i) {
      set(fresh_, nfresh_, list[i], false);
      open_[list[i]] = 0;
      set(mark_, nmark_, list[i], false);
    }
  }
  // mhpc_update_problems: a gait step rotates the nominal, which is then no longer k_init's
  void stepped(int b) { set(fresh_, nfresh_, b, false); }
  // mhpc_reset_problems of problem b
  void reset(int b, bool no_al) {
    set(fresh_, nfresh_, b, true);
    open_[b] = no_al;
  }
  // mhpc_copy_problems: problem d becomes src's problem s (src may be this ledger).  No command is
  // pending in either handle then, so no mark moves.
  void copied(int d, const Ledger& src, int s) { copied(d, src.fresh_[s] != 0, src.open_[s] != 0); }
  // ... or the marks a snapshot entry carries (mhpc_restore_problems)
  void copied(int d, bool fresh, bool open) {
    set(fresh_, nfresh_, d, fresh);
    open_[d] = open;
  }
  void command_changed(int b) { set(mark_, nmark_, b, true); }
  // mhpc_initialize / mhpc_update_problem(s): every problem's references are current
  void all_current() { fill(mark_, nmark_, false); }
  // mhpc_set_option_sets gave problem b AL iterations.  If its SRB nominal is open, its next
  // solve's first forward_sweep(0) is the reference's real rollout, not the cost evaluation of a
  // nominal k_init completed.  no_rollout_due (right after mhpc_initialize: nothing solved): that
  // solve starts with the rollout for b and with the cost evaluation for everybody else -- all
  // fresh, then b not -- and true is returned: the caller's solve must start with the rollout.
  // Otherwise it starts with the rollout anyway and b only stops being fresh.
  bool budget_raised(int b, bool no_rollout_due) {
    if (!open_[b]) return false;
    open_[b] = 0;
    if (no_rollout_due) fill(fresh_, nfresh_, true);
    set(fresh_, nfresh_, b, false);
    return no_rollout_due;
  }
  // mhpc_import_plan(_device) wrote a guess into problem b's nominal: the controls are no longer
  // the ones its trajectory was rolled out with, so its next solve's first forward_sweep(0) is the
  // real rollout, as after a gait step.  Same shape as budget_raised.  no_rollout_due (the handle
  // initialised, nothing solved, no rollout pending): that solve starts with the rollout for b and
  // with the cost evaluation for everybody else -- all fresh, then b not -- and true is returned:
  // the caller's solve must start with the rollout.  Otherwise -- a rollout is due anyway (after
  // mhpc_update_problem(s), an earlier guess), or a solve ran (mhpc_tick_problems rolls out every
  // problem that is not fresh) -- b only stops being fresh.
  // `open` is left alone: a problem whose record has no AL iteration never rolls anything out, in
  // the reference either (MultiPhaseDDP::solve's loop does not run), so its guess stays as written
  // and its SRB nominal is still the one k_init left.
  bool guessed(int b, bool no_rollout_due) {
    if (no_rollout_due) fill(fresh_, nfresh_, true);
    set(fresh_, nfresh_, b, false);
    return no_rollout_due;
  }
};

}  // namespace MHPC_NS
