// mhpc_locomotion.hpp -- C++ host surface of the reference controller over the C-ABI.
//
// Same names, fields and defaults as the reference's API so that the reference's driver
// (test_main.cpp:12-35) compiles against it unchanged except for the include:
//   HSDDP_OPTION<T>        MHPC_CompoundTypes.h:196-212
//   USRCMD                 MHPC_CompoundTypes.h:237-240
//   MHPCUserParameters     MHPC_CompoundTypes.h:242-251  (alias MHPC_UserParameter)
//   GaitType2D, Gait       Gait.h:6-77
//   MHPCLocomotion<T>      MHPCLocomotion.h:13-83 (initialization, solve_mhpc, print_debugInfo)
//   MultiPhaseDDP<T>       MultiPhaseDDP.h:12-63 (public _phases, _n_phases, _option,
//                          _actual_cost, _exp_cost_change, _tconstr_violation)
//   SinglePhaseAbstract<T> SinglePhaseAbstract.h:66-134 (public _modeidx, _phaseidx, _dt,
//                          _N_TIMESTEPS, _V, _dV, _xsize/_usize/_ysize, get_modeidx,
//                          get_nominal_ms_ptr, get_CTG_info_ptr, get_terminal_state)
//   ModelState, CostToGoStruct  MHPC_CompoundTypes.h:7-22,88-114 (x/u/y; G, du, K)
// The heavy lifting happens in libmhpc_amd.so (HIP, gfx950).  Extensions: a batch of
// independent problems per object, and set_initial_conditions() for per-problem x0.
// Header-only; link with -lmhpc_amd.  Errors throw std::runtime_error on this side of
// the ABI (none cross it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "mhpc_capi.h"

template <typename T>
struct HSDDP_OPTION {
  T alpha = 0.1;
  T gamma = 0.01;
  T update_penalty = 8;
  T update_relax = 0.1;
  T update_regularization = 2;
  T update_ReB = 7;
  T max_DDP_iter = 3;
  T max_AL_iter = 2;
  T DDP_thresh = 1e-03;
  T AL_thresh = 1e-03;
  bool AL_active = 1;
  bool ReB_active = 1;
  bool smooth_active = 0;
};

struct USRCMD {
  float vel, height, roll, pitch, yaw;
};

struct MHPCUserParameters {
  int n_wbphase = 4;
  int n_fbphase = 4;
  float dt_wb = .001;
  float dt_fb = .001;
  int cmode = 1;
  float groundH = -0.404;  // unused, as in the reference (ground hard-coded at -0.404)
  USRCMD* usrcmd = nullptr;
};
using MHPC_UserParameter = MHPCUserParameters;

enum class GaitType2D { STAND, BOUND, PRONK };

class Gait {
 public:
  Gait() : mode_{1, 2, 3, 4}, timing_{0.08f, 0.1f, 0.08f, 0.1f} {}
  explicit Gait(GaitType2D g) : mode_{1, 2, 3, 4} {
    if (g == GaitType2D::BOUND) timing_ = {0.08f, 0.1f, 0.08f, 0.1f};
    else timing_ = {0.08f, 0.08f, 0.08f, 0.08f};  // default branch of the reference switch
  }
  int get_next_mode(int current_mode) const {
    for (size_t i = 0; i < mode_.size(); ++i)
      if (mode_[i] == current_mode) return mode_[(i + 1) % mode_.size()];
    throw std::runtime_error("mode not in gait");
  }
  std::vector<int> get_mode_seq(int current_mode, int num_phases) const {
    std::vector<int> s(num_phases);
    s[0] = current_mode;
    for (int p = 0; p + 1 < num_phases; ++p) s[p + 1] = get_next_mode(s[p]);
    return s;
  }
  std::vector<float> get_timings(const std::vector<int>& seq) const {
    std::vector<float> t(seq.size());
    for (size_t i = 0; i < seq.size(); ++i) t[i] = timing_[seq[i] - 1];
    return t;
  }
  mhpc_gait to_c() const {
    mhpc_gait g{};
    g.n_modes = (int)mode_.size();
    for (size_t i = 0; i < mode_.size(); ++i) g.modes[i] = mode_[i];
    for (size_t i = 0; i < timing_.size(); ++i) g.timings[i] = timing_[i];
    return g;
  }

 private:
  std::vector<int> mode_;
  std::vector<float> timing_;
};

// Fixed-size vector / matrix with Eigen's element access (v(i), v[i], m(r, c); m stored
// column-major like Eigen's default), enough for reading solver output the way the
// reference's callers read VecM / MatMN (MHPC_CPPTypes.h).
template <typename T, size_t n>
struct VecM {
  T v[n] = {};
  T& operator()(size_t i) { return v[i]; }
  const T& operator()(size_t i) const { return v[i]; }
  T& operator[](size_t i) { return v[i]; }
  const T& operator[](size_t i) const { return v[i]; }
  static constexpr size_t size() { return n; }
  T* data() { return v; }
  const T* data() const { return v; }
};
template <typename T, size_t r, size_t c>
struct MatMN {
  T v[r * c] = {};
  T& operator()(size_t i, size_t j) { return v[j * r + i]; }
  const T& operator()(size_t i, size_t j) const { return v[j * r + i]; }
  static constexpr size_t rows() { return r; }
  static constexpr size_t cols() { return c; }
  T* data() { return v; }
  const T* data() const { return v; }
};

// One knot of a phase's nominal trajectory (MHPC_CompoundTypes.h:7-22)
template <typename T, size_t xsize, size_t usize, size_t ysize>
struct ModelState {
  VecM<T, xsize> x;
  VecM<T, usize> u;
  VecM<T, ysize> y;
};

// One knot of a phase's cost-to-go information (MHPC_CompoundTypes.h:88-101): the value
// gradient G (Vx) and the feedback du, K that the execution horizon consumes.  The Hessian H
// and the Q-function blocks are intermediates of the backward sweep that the device keeps
// in LDS and never writes to HBM; they are not part of this struct (reading them fails to
// compile instead of returning zeros).
template <typename T, size_t xsize, size_t usize>
struct CostToGoStruct {
  VecM<T, xsize> G;
  VecM<T, usize> du;
  MatMN<T, usize, xsize> K;
};

// Read-only view of one phase of one problem of the batch after a solve, with the public
// members and accessors of the reference's SinglePhaseAbstract (SinglePhaseAbstract.h:66-134).
// The nominal / cost-to-go arrays are copied from the device on first access after a solve.
template <typename T>
class SinglePhaseAbstract {
 public:
  int _modeidx = 1;
  int _phaseidx = 1;
  T _dt = 0;
  size_t _N_TIMESTEPS = 0;
  T _V = 0;   // actual cost of this phase only
  T _dV = 0;  // expected cost change of this phase
  size_t _xsize = 0, _usize = 4, _ysize = 4;

  size_t get_modeidx() const { return _modeidx; }
  // ModelState<T, _xsize, 4, 4>[_N_TIMESTEPS] (cast as the reference's solve_mhpc does)
  void* get_nominal_ms_ptr() { fetch(); return ms_.data(); }
  // CostToGoStruct<T, _xsize, 4>[_N_TIMESTEPS]
  void* get_CTG_info_ptr() { fetch(); return ctg_.data(); }
  std::vector<T> get_terminal_state() {
    fetch();
    const T* xN = ms_.data() + (_N_TIMESTEPS - 1) * ms_stride();
    return std::vector<T>(xN, xN + _xsize);
  }

 private:
  template <typename>
  friend class MHPCLocomotion;
  size_t ms_stride() const {
    return _xsize == 14 ? sizeof(ModelState<T, 14, 4, 4>) / sizeof(T)
                        : sizeof(ModelState<T, 6, 4, 4>) / sizeof(T);
  }
  size_t ctg_stride() const {
    return _xsize == 14 ? sizeof(CostToGoStruct<T, 14, 4>) / sizeof(T)
                        : sizeof(CostToGoStruct<T, 6, 4>) / sizeof(T);
  }
  void fetch() {
    if (!stale_) return;
    const size_t n = _xsize, N = _N_TIMESTEPS;
    std::vector<double> x(N * n), u(N * 4), y(N * 4), K(N * 4 * n), du(N * 4), G(N * n);
    const int rc = mhpc_get_phase_problems(h_, phase_, problem_, 1, x.data(), u.data(), y.data(),
                                           K.data(), du.data(), G.data());
    if (rc != MHPC_OK)
      throw std::runtime_error(std::string("mhpc_get_phase_problems: ") + mhpc_last_error());
    const size_t ms = ms_stride(), cs = ctg_stride();
    ms_.assign(N * ms, T(0));
    ctg_.assign(N * cs, T(0));
    for (size_t k = 0; k < N; ++k) {
      T* m = &ms_[k * ms];  // x, u, y contiguous (ModelState's member order)
      for (size_t i = 0; i < n; ++i) m[i] = (T)x[k * n + i];
      for (size_t i = 0; i < 4; ++i) m[n + i] = (T)u[k * 4 + i];
      for (size_t i = 0; i < 4; ++i) m[n + 4 + i] = (T)y[k * 4 + i];
      T* c = &ctg_[k * cs];  // G, du, K (column-major 4 x n)
      for (size_t i = 0; i < n; ++i) c[i] = (T)G[k * n + i];
      for (size_t i = 0; i < 4; ++i) c[n + i] = (T)du[k * 4 + i];
      for (size_t r = 0; r < 4; ++r)
        for (size_t j = 0; j < n; ++j) c[n + 4 + j * 4 + r] = (T)K[(k * 4 + r) * n + j];
    }
    stale_ = false;
  }
  mhpc_handle* h_ = nullptr;
  int phase_ = 0, problem_ = 0;
  bool stale_ = true;
  std::vector<T> ms_, ctg_;
};

template <typename TH>
class MHPCLocomotion {
 public:
  // MHPCLocomotion(MHPCUserParameters*, Gait*, HSDDP_OPTION<TH>)  (MHPCLocomotion.cpp:8-43)
  MHPCLocomotion(MHPCUserParameters* params, Gait* gait, HSDDP_OPTION<TH> option, int batch = 1,
                 int device = 0)
      : batch_(batch) {
    static_assert(sizeof(TH) == 8, "only the double instantiation exists (as in the reference)");
    const int np = params->n_wbphase + params->n_fbphase;
    desc_ = build_desc(params, gait);
    opt_ = option_to_c(option);
    check(mhpc_create(&desc_, &opt_, batch_, device, &h_), "mhpc_create");
    _option = option;
    _n_phases = np;
    gait_ = gait->to_c();
    // default initial condition (MHPCLocomotion.cpp:37-39), projected if phase 0 is SRB
    const double x0[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                           0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
    xw_ = desc_.n_wb > 0 ? 14 : 6;
    pmax_ = np;
    refresh_phases(false);
    default_x0();
  }
  ~MHPCLocomotion() { mhpc_destroy(h_); }
  // the phase layout MHPCLocomotion::build_problem makes (MHPCLocomotion.cpp:63-104) for the
  // controller's parameters and gait at its current mode params->cmode
  static mhpc_problem_desc build_desc(const MHPCUserParameters* params, Gait* gait) {
    const int np = params->n_wbphase + params->n_fbphase;
    mhpc_problem_desc d{};
    d.n_wb = params->n_wbphase;
    d.n_fb = params->n_fbphase;
    d.dt_wb = (double)params->dt_wb;
    d.dt_fb = (double)params->dt_fb;
    d.vel_cmd = params->usrcmd ? params->usrcmd->vel : 0.f;
    d.height_cmd = params->usrcmd ? params->usrcmd->height : 0.f;
    d.precision = 64;
    const std::vector<int> seq = gait->get_mode_seq(params->cmode, np);
    const std::vector<float> tim = gait->get_timings(seq);
    for (int p = 0; p < np && p < MHPC_MAX_PHASES; ++p) {
      d.mode_seq[p] = seq[p];
      // float timing / (double)(float dt), as the reference's DVec<float> / double member
      d.N[p] = (int)std::round((double)tim[p] / (p < d.n_wb ? d.dt_wb : d.dt_fb));
    }
    return d;
  }
  static mhpc_hsddp_option option_to_c(const HSDDP_OPTION<TH>& o) {
    return mhpc_hsddp_option{o.alpha, o.gamma, o.update_penalty, o.update_relax, o.update_regularization,
                             o.update_ReB, o.max_DDP_iter, o.max_AL_iter, o.DDP_thresh, o.AL_thresh,
                             o.AL_active, o.ReB_active, o.smooth_active, 0};
  }
  static HSDDP_OPTION<TH> option_from_c(const mhpc_hsddp_option& c) {
    HSDDP_OPTION<TH> o;
    o.alpha = c.alpha; o.gamma = c.gamma; o.update_penalty = c.update_penalty;
    o.update_relax = c.update_relax; o.update_regularization = c.update_regularization;
    o.update_ReB = c.update_ReB; o.max_DDP_iter = c.max_DDP_iter; o.max_AL_iter = c.max_AL_iter;
    o.DDP_thresh = c.DDP_thresh; o.AL_thresh = c.AL_thresh; o.AL_active = c.AL_active != 0;
    o.ReB_active = c.ReB_active != 0; o.smooth_active = c.smooth_active != 0;
    return o;
  }
  MHPCLocomotion(const MHPCLocomotion&) = delete;
  MHPCLocomotion& operator=(const MHPCLocomotion&) = delete;

  // extension: per-problem initial states [batch][x0_width()] (14 when any problem has a
  // whole-body phase -- an SRB-only problem reads the first 6 of its row -- else 6)
  void set_initial_conditions(const std::vector<double>& x0) {
    x0_ = x0;
    x0_on_device_ = false;
  }
  int x0_width() const { return xw_; }
  // MultiPhaseDDP::set_initial_condition for every problem of the batch (same state)
  void set_initial_condition(const std::vector<double>& x0) {
    for (int b = 0; b < batch_; ++b)
      for (int i = 0; i < xw_; ++i) x0_[(size_t)b * xw_ + i] = x0[i];
    x0_on_device_ = false;
  }

  // MHPCLocomotion::update_problem (MHPCLocomotion.cpp:107-158): gait advances one mode,
  // phase buffers rotate (warm start), references follow the current initial condition
  void update_problem() {
    push_x0();
    check(mhpc_update_problem(h_, &gait_), "mhpc_update_problem");
    refresh_descs();
  }

  // extension: per-problem phase layouts in one batch -- one MHPCLocomotion per controller
  // in the reference, each built from its own Gait / gait point (MHPCLocomotion.cpp:63-104).
  // Problem b gets descs[layout_of_problem[b]] (descs[b % n] for an empty vector); the
  // initial states return to the default, initialization() precedes the next solve.
  void set_layouts(const std::vector<mhpc_problem_desc>& descs,
                   const std::vector<int32_t>& layout_of_problem = {}) {
    check(mhpc_set_layouts(h_, (int)descs.size(), descs.data(),
                           layout_of_problem.empty() ? nullptr : layout_of_problem.data()),
          "mhpc_set_layouts");
    refresh_descs();
    default_x0();
  }
  // extension: update_problem per controller -- problem b takes steps[b] gait steps of
  // gaits[gait_of_problem[b]] (0: keeps its layout and warm start); empty vectors: gaits[0]
  // for every problem, one step each
  void update_problems(const std::vector<Gait*>& gaits,
                       const std::vector<int32_t>& gait_of_problem = {},
                       const std::vector<int32_t>& steps = {}) {
    std::vector<mhpc_gait> gs;
    for (Gait* g : gaits) gs.push_back(g->to_c());
    push_x0();
    check(mhpc_update_problems(h_, (int)gs.size(), gs.data(),
                               gait_of_problem.empty() ? nullptr : gait_of_problem.data(),
                               steps.empty() ? nullptr : steps.data()),
          "mhpc_update_problems");
    refresh_descs();
  }
  // extension: initialization() of the listed problems only -- set_initial_condition +
  // initialization() on one controller of a fleet (MHPCLocomotion.cpp:47-53), the others keep
  // their warm start bit for bit.  x0 [problems.size()][x0_width()] in list order, empty: each
  // listed problem keeps its current device row.  After a solve, follow with update_problems
  // (steps 0 for the reset problems); before a solve, just solve.
  void reset_problems(const std::vector<int>& problems, const std::vector<double>& x0 = {}) {
    if (!x0.empty() && x0.size() != problems.size() * (size_t)xw_)
      throw std::runtime_error("reset_problems: x0 must be [problems][x0_width()]");
    const std::vector<int32_t> pr(problems.begin(), problems.end());
    check(mhpc_reset_problems(h_, (int)pr.size(), pr.data(), x0.empty() ? nullptr : x0.data(), 0,
                              nullptr, nullptr),
          "mhpc_reset_problems");
    for (size_t i = 0; i < pr.size() && !x0.empty(); ++i)  // what update_problem(s) hands back
      std::copy(x0.begin() + i * xw_, x0.begin() + (i + 1) * xw_, x0_.begin() + (size_t)pr[i] * xw_);
    refresh_descs();
  }
  // extension: one MPC tick of the listed problems and of nobody else -- set_initial_condition +
  // update_problem + solve_mhpc on single controllers of a fleet, each when its own gait mode ends
  // (mhpc_tick_problems).  x0 [problems.size()][x0_width()] in list order, empty: each listed
  // problem keeps its current device row; listed problem i takes steps[i] gait steps (empty: one
  // each) of gaits[gait_of[i]] (empty: gaits[0]; no gaits: this controller's own gait).  Every
  // other problem keeps its state bit for bit.  Returns the listed problems' status in list order
  // (also kept in status()); ms: the device time of the whole tick.
  std::vector<int32_t> tick_problems(const std::vector<int>& problems, const std::vector<double>& x0 = {},
                                     const std::vector<Gait*>& gaits = {},
                                     const std::vector<int32_t>& gait_of = {},
                                     const std::vector<int32_t>& steps = {}, float* ms = nullptr) {
    if (!x0.empty() && x0.size() != problems.size() * (size_t)xw_)
      throw std::runtime_error("tick_problems: x0 must be [problems][x0_width()]");
    if ((!gait_of.empty() && gait_of.size() != problems.size()) ||
        (!steps.empty() && steps.size() != problems.size()))
      throw std::runtime_error("tick_problems: one gait index / step count per listed problem");
    const std::vector<int32_t> pr(problems.begin(), problems.end());
    std::vector<mhpc_gait> gs;
    for (Gait* g : gaits) gs.push_back(g->to_c());
    if (gs.empty()) gs.push_back(gait_);
    std::vector<int32_t> st(pr.size(), 0);
    check(mhpc_tick_problems(h_, (int)pr.size(), pr.data(), x0.empty() ? nullptr : x0.data(),
                             (int)gs.size(), gs.data(), gait_of.empty() ? nullptr : gait_of.data(),
                             steps.empty() ? nullptr : steps.data(), st.data(), ms),
          "mhpc_tick_problems");
    status_.resize(batch_, 0);
    for (size_t i = 0; i < pr.size(); ++i) {
      status_[pr[i]] = st[i];
      if (!x0.empty() && !x0_on_device_)  // what update_problem(s) hands back
        std::copy(x0.begin() + i * xw_, x0.begin() + (i + 1) * xw_, x0_.begin() + (size_t)pr[i] * xw_);
    }
    refresh_descs();
    refresh_phases(true);
    return st;
  }
  // extension: floor of the knot stride of the packed arrays, so that later ticks can step into
  // longer layouts (mhpc_reserve_knots); before initialization()
  void reserve_knots(int knots) { check(mhpc_reserve_knots(h_, knots), "mhpc_reserve_knots"); }
  // extension: copying controller objects -- problem dst_problems[i] of this fleet becomes a copy
  // of problem src_problems[i] of `src` (nullptr: of this fleet) as it stands: warm start, solver
  // state, x0 row, command, parameter set, layout and phase buffers.  A source may repeat (one
  // robot forks into several candidates); every other problem keeps its state bit for bit.
  // Returns the device time of the copy in ms.
  float copy_problems(const std::vector<int>& dst_problems, const std::vector<int>& src_problems,
                      MHPCLocomotion* src = nullptr) {
    if (dst_problems.size() != src_problems.size())
      throw std::runtime_error("copy_problems: one source problem per destination problem");
    if (!src) src = this;
    const std::vector<int32_t> dp(dst_problems.begin(), dst_problems.end());
    const std::vector<int32_t> sp(src_problems.begin(), src_problems.end());
    float ms = 0;
    check(mhpc_copy_problems(h_, dp.data(), src->h_, sp.data(), (int)dp.size(), &ms),
          "mhpc_copy_problems");
    const std::vector<double> rows = get_x0();  // what update_problem(s) hands back
    status_.resize(batch_, 0);
    for (size_t i = 0; i < dp.size(); ++i) {
      std::copy(rows.begin() + (size_t)dp[i] * xw_, rows.begin() + (size_t)(dp[i] + 1) * xw_,
                x0_.begin() + (size_t)dp[i] * xw_);
      status_[dp[i]] = (size_t)sp[i] < src->status_.size() ? src->status_[sp[i]] : 0;
    }
    refresh_descs();
    return ms;
  }
  // extension: snapshots -- the copy above, serialised (mhpc_snapshot_problems).  The listed
  // problems (empty: all) as they stand, as a blob of plain bytes that restore_problems /
  // from_snapshot turn back into live problems of this or any other fleet, in any process.
  std::vector<uint8_t> snapshot_problems(const std::vector<int>& problems = {}, float* ms = nullptr) {
    std::vector<int32_t> pr(problems.begin(), problems.end());
    if (pr.empty())
      for (int b = 0; b < batch_; ++b) pr.push_back(b);
    int64_t bytes = 0;
    check(mhpc_snapshot_size(h_, (int)pr.size(), pr.data(), &bytes), "mhpc_snapshot_size");
    std::vector<uint8_t> blob((size_t)bytes);
    check(mhpc_snapshot_problems(h_, (int)pr.size(), pr.data(), blob.data(), bytes, ms),
          "mhpc_snapshot_problems");
    return blob;
  }
  // problem dst_problems[i] becomes entry entries[i] of the blob (empty: entry i); an entry may
  // repeat.  A restore that lists every problem also adopts the blob's point of the call order.
  // Returns the device time of the unpack launches in ms.
  float restore_problems(const std::vector<int>& dst_problems, const std::vector<uint8_t>& blob,
                         const std::vector<int>& entries = {}) {
    if (!entries.empty() && entries.size() != dst_problems.size())
      throw std::runtime_error("restore_problems: one blob entry per destination problem");
    const std::vector<int32_t> dp(dst_problems.begin(), dst_problems.end());
    const std::vector<int32_t> en(entries.begin(), entries.end());
    float ms = 0;
    check(mhpc_restore_problems(h_, (int)dp.size(), dp.data(), blob.data(), (int64_t)blob.size(),
                                en.empty() ? nullptr : en.data(), &ms),
          "mhpc_restore_problems");
    const std::vector<double> rows = get_x0();  // what update_problem(s) hands back
    status_.resize(batch_, 0);
    for (size_t i = 0; i < dp.size(); ++i) {
      std::copy(rows.begin() + (size_t)dp[i] * xw_, rows.begin() + (size_t)(dp[i] + 1) * xw_,
                x0_.begin() + (size_t)dp[i] * xw_);
      check(mhpc_snapshot_status(blob.data(), (int64_t)blob.size(), en.empty() ? (int)i : en[i], 1,
                                 &status_[dp[i]]),
            "mhpc_snapshot_status");
    }
    refresh_descs();
    _option = get_options();
    return ms;
  }
  static struct mhpc_snapshot_info snapshot_info(const std::vector<uint8_t>& blob) {
    struct mhpc_snapshot_info info;
    check(::mhpc_snapshot_info(blob.data(), (int64_t)blob.size(), &info), "mhpc_snapshot_info");
    return info;
  }
  struct SnapshotEntry {
    mhpc_problem_desc desc;  // with the entry's command
    mhpc_hsddp_option option;
    mhpc_cost_weights weights;
    mhpc_constraint_params constraints;
  };
  static SnapshotEntry snapshot_entry(const std::vector<uint8_t>& blob, int i) {
    SnapshotEntry e;
    check(mhpc_snapshot_entry(blob.data(), (int64_t)blob.size(), i, &e.desc, &e.option, &e.weights,
                              &e.constraints),
          "mhpc_snapshot_entry");
    return e;
  }
  // A fleet that can hold the blob and holds it: the entries' descriptors (set_layouts), their
  // longest layout as reserve_knots, the blob's alpha, precision and sweep arithmetic, the distinct
  // option records (set_option_sets); initialised, every entry restored into problems 0..n-1.
  // batch 0: the entry count, so the fleet resumes at the blob's point of the call order.  gait:
  // what update_problem() steps with (a blob holds gait points, not gaits).
  static std::unique_ptr<MHPCLocomotion> from_snapshot(const std::vector<uint8_t>& blob, Gait* gait,
                                                       int device = 0, int batch = 0) {
    const struct mhpc_snapshot_info info = snapshot_info(blob);
    const int n = info.n_entries, B = batch > 0 ? batch : n;
    if (B < n) throw std::runtime_error("from_snapshot: batch smaller than the blob's entry count");
    std::vector<mhpc_problem_desc> descs;
    std::vector<mhpc_hsddp_option> opts;
    std::vector<int32_t> lop(B, 0), oop(B, 0);
    for (int i = 0; i < n; ++i) {
      SnapshotEntry e = snapshot_entry(blob, i);
      if (i > 0) {  // one handle-wide command in the descriptors: the entries' own travel with them
        e.desc.vel_cmd = descs[0].vel_cmd;
        e.desc.height_cmd = descs[0].height_cmd;
      }
      size_t k = 0;
      while (k < descs.size() && std::memcmp(&descs[k], &e.desc, sizeof e.desc) != 0) ++k;
      if (k == descs.size()) descs.push_back(e.desc);
      lop[i] = (int32_t)k;
      for (k = 0; k < opts.size() && std::memcmp(&opts[k], &e.option, sizeof e.option) != 0;) ++k;
      if (k == opts.size()) opts.push_back(e.option);
      oop[i] = (int32_t)k;
    }
    std::unique_ptr<MHPCLocomotion> f(new MHPCLocomotion(descs[0], opts[0], gait, B, device));
    if (info.sweep_bits == 32)
      check(mhpc_set_kernel_variant(f->h_, MHPC_VARIANT_SWEEP_BITS, 32), "mhpc_set_kernel_variant");
    if (descs.size() > 1) f->set_layouts(descs, lop);
    f->reserve_knots(info.knot_stride);
    if (opts.size() > 1) {
      check(mhpc_set_option_sets(f->h_, (int)opts.size(), opts.data(), oop.data()), "mhpc_set_option_sets");
      f->_option = f->get_options();
    }
    f->initialization();
    std::vector<int> all(n);
    for (int i = 0; i < n; ++i) all[i] = i;
    f->restore_problems(all, blob);
    return f;
  }
  // thin file helpers over the two
  void save_problems(const std::string& path, const std::vector<int>& problems = {}) {
    const std::vector<uint8_t> blob = snapshot_problems(problems);
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)blob.data(), (std::streamsize)blob.size());
    if (!f) throw std::runtime_error("save_problems: cannot write " + path);
  }
  static std::vector<uint8_t> load_snapshot(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("load_snapshot: cannot read " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  }
  // problems whose last solve did not end MHPC_SOLVE_OK or left a non-finite cost
  std::vector<int> lost_problems() {
    std::vector<double> J(batch_);
    check(mhpc_get_scalars(h_, J.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
          "mhpc_get_scalars");
    std::vector<int> lost;
    for (int b = 0; b < batch_; ++b)
      if ((b < (int)status_.size() && status_[b] != MHPC_SOLVE_OK) || !std::isfinite(J[b]))
        lost.push_back(b);
    return lost;
  }
  // extension: per-problem user commands in one batch -- the usrcmd (float vel, height) of one
  // controller per problem, which build_problem hands to ReferenceGen (MHPCLocomotion.cpp
  // :98-103).  One entry per problem, an empty vector keeps the current values; they take
  // effect at the next initialization() / update_problem(s), and an initialised object refuses
  // to solve until then.
  void set_commands(const std::vector<float>& vel, const std::vector<float>& height = {}) {
    if ((!vel.empty() && (int)vel.size() != batch_) ||
        (!height.empty() && (int)height.size() != batch_))
      throw std::runtime_error("set_commands: one entry per problem expected");
    const std::vector<double> v(vel.begin(), vel.end()), hg(height.begin(), height.end());
    check(mhpc_set_commands(h_, v.empty() ? nullptr : v.data(), hg.empty() ? nullptr : hg.data()),
          "mhpc_set_commands");
  }
  void get_commands(std::vector<double>& vel, std::vector<double>& height) {
    vel.assign(batch_, 0.0);
    height.assign(batch_, 0.0);
    check(mhpc_get_commands(h_, vel.data(), height.data()), "mhpc_get_commands");
  }
  // extension: the solved feedback policy u = u_nom + K (x - x_nom) run from measured or
  // perturbed start states -- the reference's set_initial_condition(x) followed by
  // forward_sweep_dynamics_only(0) (SinglePhase.cpp:117-144, MultiPhaseDDP.cpp:56-76), for
  // n_samples states per problem in one launch.  xs [batch][n_samples][x0_width()]; n_phases
  // phases are rolled (0: every phase of each problem).  J, viol [batch][n_samples], x_end
  // [batch][n_samples][x0_width()]: the state after the last rolled phase's transition
  // (post-impact whole-body state, usable as the next x0).  Nothing is modified.
  struct PolicyRollout { int n_samples = 0; std::vector<double> J, viol, x_end; float ms = 0; };
  PolicyRollout rollout_policy(const std::vector<double>& xs, int n_phases = 0) {
    const size_t row = (size_t)batch_ * xw_;
    if (xs.empty() || xs.size() % row != 0)
      throw std::runtime_error("rollout_policy: xs must be [batch][n_samples][x0_width()]");
    PolicyRollout r;
    r.n_samples = (int)(xs.size() / row);
    const size_t n = (size_t)batch_ * r.n_samples;
    r.J.assign(n, 0.0);
    r.viol.assign(n, 0.0);
    r.x_end.assign(n * xw_, 0.0);
    check(mhpc_rollout_policy(h_, r.n_samples, xs.data(), n_phases, r.J.data(), r.viol.data(),
                              r.x_end.data(), &r.ms),
          "mhpc_rollout_policy");
    return r;
  }
  // trajectories of phase p under the policy (rolled from phase 0) for problems
  // [first, first + count): x [count][n_samples][N][xsize], u, y [count][n_samples][N][4]
  // (the range's phase must have one shape); xs [count][n_samples][x0_width()]
  struct PolicyPhase { int n_samples = 0, N = 0, xsize = 0; std::vector<double> x, u, y; };
  PolicyPhase rollout_policy_phase(int p, int first, int count, const std::vector<double>& xs) {
    const size_t row = (size_t)count * xw_;
    if (count < 1 || xs.empty() || xs.size() % row != 0)
      throw std::runtime_error("rollout_policy_phase: xs must be [count][n_samples][x0_width()]");
    PolicyPhase r;
    r.n_samples = (int)(xs.size() / row);
    const mhpc_problem_desc d = problem_desc(first);
    check(mhpc_phase_dims(&d, p, &r.xsize, &r.N), "mhpc_phase_dims");
    const size_t n = (size_t)count * r.n_samples * r.N;
    r.x.assign(n * r.xsize, 0.0);
    r.u.assign(n * 4, 0.0);
    r.y.assign(n * 4, 0.0);
    check(mhpc_rollout_policy_phase(h_, p, first, count, r.n_samples, xs.data(), r.x.data(),
                                    r.u.data(), r.y.data()),
          "mhpc_rollout_policy_phase");
    return r;
  }
  // device-side closed loop: every problem's initial condition becomes the end state of one
  // policy rollout over n_phases phases from x0 + dx (dx [batch][x0_width()], empty: zero), with
  // no host copy of states; update_problem() / initialization() follow as after
  // set_initial_conditions()
  void advance_x0(int n_phases = 1, const std::vector<double>& dx = {}) {
    if (!dx.empty() && dx.size() != (size_t)batch_ * xw_)
      throw std::runtime_error("advance_x0: dx must be [batch][x0_width()]");
    check(mhpc_advance_x0(h_, n_phases, dx.empty() ? nullptr : dx.data()), "mhpc_advance_x0");
    x0_on_device_ = true;  // update_problem() / initialization() push nothing over the rows
  }
  // the device's current initial states [batch][x0_width()]
  std::vector<double> get_x0() {
    std::vector<double> x0((size_t)batch_ * xw_);
    check(mhpc_get_x0(h_, x0.data()), "mhpc_get_x0");
    return x0;
  }
  // ---- device-resident control I/O: measured states in, feedback controls out ---------------
  // control steps of problem b: the knots with a control of its whole-body phases, or of all its
  // phases when it is SRB-only (mhpc_num_control_steps)
  int num_control_steps(int b = 0) {
    int n = 0;
    check(mhpc_num_control_steps(h_, b, &n), "mhpc_num_control_steps");
    return n;
  }
  // u = u_nom + K (x - x_nom) of every problem at control step step[b] (empty: step 0) from its
  // measured state x [batch][x0_width()], one knot of forward_sweep_dynamics_only
  // (SinglePhase.cpp:117-144), the policy rollouts' arithmetic bit for bit (mhpc_control):
  // u [batch][4]; with_policy: also x_nom [batch][x0_width()], u_nom [batch][4],
  // K [batch][4][x0_width()]
  struct Control { std::vector<double> u, x_nom, u_nom, K; };
  Control control(const std::vector<int32_t>& step, const std::vector<double>& x,
                  bool with_policy = false) {
    if (x.size() != (size_t)batch_ * xw_ || (!step.empty() && step.size() != (size_t)batch_))
      throw std::runtime_error("control: x must be [batch][x0_width()], step [batch] or empty");
    Control c;
    c.u.assign((size_t)batch_ * 4, 0.0);
    if (with_policy) {
      c.x_nom.assign((size_t)batch_ * xw_, 0.0);
      c.u_nom.assign((size_t)batch_ * 4, 0.0);
      c.K.assign((size_t)batch_ * 4 * xw_, 0.0);
    }
    check(mhpc_control(h_, step.empty() ? nullptr : step.data(), x.data(), c.u.data(),
                       with_policy ? c.x_nom.data() : nullptr, with_policy ? c.u_nom.data() : nullptr,
                       with_policy ? c.K.data() : nullptr),
          "mhpc_control");
    return c;
  }
  // the same on device arrays of the caller's (mhpc_control_device): x rows of x0_width() at a
  // stride of ldx elements, u rows of 4 at ldu, of dtype MHPC_DEV_F64 / MHPC_DEV_F32 (slices of a
  // simulator's state / action tensors); ordered after everything queued on `stream` (the
  // caller's hipStream_t, null: the null stream), finished when the call returns
  void control_device(const std::vector<int32_t>& step, const void* x, int64_t ldx, void* u,
                      int64_t ldu, int dtype = MHPC_DEV_F64, void* stream = nullptr,
                      void* x_nom = nullptr, void* u_nom = nullptr, void* K = nullptr) {
    if (!step.empty() && step.size() != (size_t)batch_)
      throw std::runtime_error("control_device: step must be [batch] or empty");
    check(mhpc_control_device(h_, step.empty() ? nullptr : step.data(), x, ldx, u, ldu, x_nom, u_nom,
                              K, dtype, stream),
          "mhpc_control_device");
  }
  // `window` control steps of each listed problem's policy from first_step[i] (empty: 0) into the
  // device arrays `out` names (mhpc_export_plan_device): row i belongs to problems[i] (empty: the
  // whole batch in order), rows past valid[i] and columns past a problem's state size are +0, every
  // value is what mhpc_get_phase_problems reports for the step's knot.  Returns the device ms of
  // the launch.  Ordered after everything queued on `stream`, finished when the call returns.
  float export_plan_device(const std::vector<int32_t>& problems, const std::vector<int32_t>& first_step,
                           int window, const mhpc_plan_out& out, int dtype = MHPC_DEV_F64,
                           void* stream = nullptr) {
    const int n = problems.empty() ? batch_ : (int)problems.size();
    if (!first_step.empty() && first_step.size() != (size_t)n)
      throw std::runtime_error("export_plan_device: first_step must have one entry per listed problem, or none");
    float ms = 0;
    check(mhpc_export_plan_device(h_, n, problems.empty() ? nullptr : problems.data(),
                                  first_step.empty() ? nullptr : first_step.data(), window, &out,
                                  dtype, stream, &ms),
          "mhpc_export_plan_device");
    return ms;
  }
  // J, dV_exp, viol, V_phase, dV_phase (rows of max_phases) and status of the listed problems'
  // last solve into the device arrays `out` names (mhpc_export_results_device)
  void export_results_device(const std::vector<int32_t>& problems, const mhpc_results_out& out,
                             int dtype = MHPC_DEV_F64, void* stream = nullptr) {
    check(mhpc_export_results_device(h_, problems.empty() ? batch_ : (int)problems.size(),
                                     problems.empty() ? nullptr : problems.data(), &out, dtype,
                                     stream),
          "mhpc_export_results_device");
  }
  // ---- plan import: warm-start listed problems from a guess ---------------------------------
  // steps of problem b under a scope (mhpc_num_plan_steps): MHPC_STEPS_CONTROL the control steps
  // above, MHPC_STEPS_ALL every phase in order
  int num_plan_steps(int b = 0, int scope = MHPC_STEPS_CONTROL) {
    int n = 0;
    check(mhpc_num_plan_steps(h_, b, scope, &n), "mhpc_num_plan_steps");
    return n;
  }
  // `window` steps of each listed problem's nominal from first_step[i] (empty: 0) out of the
  // device arrays `in` names (mhpc_import_plan_device): u_nom, optionally K with x_nom; without K
  // the written knots' gains become +0.  The listed problems' next solve or tick starts with the
  // real rollout of the guess from x0, as after update_problem().  Returns the device ms of the
  // launch.  Ordered after everything queued on `stream`, finished when the call returns.
  float import_plan_device(const std::vector<int32_t>& problems, const std::vector<int32_t>& first_step,
                           int window, const mhpc_plan_in& in, int scope = MHPC_STEPS_CONTROL,
                           int dtype = MHPC_DEV_F64, void* stream = nullptr) {
    const int n = problems.empty() ? batch_ : (int)problems.size();
    if (!first_step.empty() && first_step.size() != (size_t)n)
      throw std::runtime_error("import_plan_device: first_step must have one entry per listed problem, or none");
    float ms = 0;
    check(mhpc_import_plan_device(h_, n, problems.empty() ? nullptr : problems.data(),
                                  first_step.empty() ? nullptr : first_step.data(), window, scope,
                                  &in, dtype, stream, &ms),
          "mhpc_import_plan_device");
    return ms;
  }
  // the same from dense host arrays (mhpc_import_plan): u_nom [n][window][4], K
  // [n][window][4][x0_width()] and x_nom [n][window][x0_width()] (both or neither); non-finite
  // entries are refused
  void import_plan(const std::vector<int32_t>& problems, const std::vector<int32_t>& first_step,
                   int window, const std::vector<double>& u_nom,
                   const std::vector<double>& K = {}, const std::vector<double>& x_nom = {},
                   int scope = MHPC_STEPS_CONTROL) {
    const size_t n = problems.empty() ? (size_t)batch_ : problems.size();
    const size_t W = window > 0 ? (size_t)window : 0;
    if (!first_step.empty() && first_step.size() != n)
      throw std::runtime_error("import_plan: first_step must have one entry per listed problem, or none");
    if (u_nom.size() != n * W * 4 || (!K.empty() && K.size() != n * W * 4 * xw_) ||
        (!x_nom.empty() && x_nom.size() != n * W * xw_))
      throw std::runtime_error("import_plan: u_nom must be [n][window][4], K [n][window][4][x0_width()], x_nom [n][window][x0_width()]");
    check(mhpc_import_plan(h_, (int)n, problems.empty() ? nullptr : problems.data(),
                           first_step.empty() ? nullptr : first_step.data(), window, scope,
                           u_nom.data(), K.empty() ? nullptr : K.data(),
                           x_nom.empty() ? nullptr : x_nom.data()),
          "mhpc_import_plan");
  }
  // set_initial_conditions from a device array, at once (mhpc_set_x0_device): rows of x0_width()
  // at x0 + b * ld; the device rows are then the current ones, update_problem() /
  // initialization() push no host copy over them
  void set_x0_device(const void* x0, int64_t ld, int dtype = MHPC_DEV_F64, void* stream = nullptr) {
    check(mhpc_set_x0_device(h_, x0, ld, dtype, stream), "mhpc_set_x0_device");
    x0_on_device_ = true;
  }

  // the tracking reference x of phase p for problems [first, first + count): [count][N][xsize]
  // (ReferenceGen.h:53-109; the range's phase must have one shape)
  std::vector<double> get_reference_problems(int p, int first, int count) {
    const mhpc_problem_desc d = problem_desc(first);
    int n = 0, N = 0;
    check(mhpc_phase_dims(&d, p, &n, &N), "mhpc_phase_dims");
    std::vector<double> xref((size_t)count * N * n);
    check(mhpc_get_reference_problems(h_, p, first, count, xref.data()),
          "mhpc_get_reference_problems");
    return xref;
  }
  mhpc_problem_desc problem_desc(int b) {
    mhpc_problem_desc d{};
    check(mhpc_get_problem_desc(h_, b, &d), "mhpc_get_problem_desc");
    return d;
  }
  int num_layouts() {
    int n = 0;
    check(mhpc_num_layouts(h_, &n), "mhpc_num_layouts");
    return n;
  }

  // execution horizon of solve_mhpc (ms_exec / CTG_exec, MHPCLocomotion.cpp:176-194): nominal
  // x [batch][Ne][14], u [batch][Ne][4], K [batch][Ne][4*14], du, G of phase 0 followed by
  // phase 1 when there are two or more WB phases (Ne = N0 (+ N1))
  struct ExecHorizon { int Ne = 0; std::vector<double> x, u, y, K, du, G; };
  ExecHorizon get_exec() {
    ExecHorizon e;
    const int np = desc_.n_wb > 1 ? 2 : 1;
    std::vector<int> Ns(np);
    for (int p = 0; p < np; ++p) Ns[p] = desc_.N[p];
    for (int p = 0; p < np; ++p) e.Ne += Ns[p];
    const size_t B = batch_, Ne = e.Ne;
    e.x.resize(B * Ne * 14); e.u.resize(B * Ne * 4); e.y.resize(B * Ne * 4);
    e.K.resize(B * Ne * 56); e.du.resize(B * Ne * 4); e.G.resize(B * Ne * 14);
    size_t off = 0;
    for (int p = 0; p < np; ++p) {
      const size_t N = Ns[p];
      std::vector<double> x(B * N * 14), u(B * N * 4), y(B * N * 4), K(B * N * 56), du(B * N * 4),
          G(B * N * 14);
      check(mhpc_get_phase(h_, p, x.data(), u.data(), y.data(), K.data(), du.data(), G.data()),
            "mhpc_get_phase");
      for (size_t b = 0; b < B; ++b) {
        auto cp = [&](std::vector<double>& dst, const std::vector<double>& src, size_t w) {
          std::copy(src.begin() + b * N * w, src.begin() + (b + 1) * N * w,
                    dst.begin() + (b * Ne + off) * w);
        };
        cp(e.x, x, 14); cp(e.u, u, 4); cp(e.y, y, 4); cp(e.K, K, 56); cp(e.du, du, 4); cp(e.G, G, 14);
      }
      off += N;
    }
    return e;
  }

  void initialization() {  // (:47-53)
    push_x0();
    check(mhpc_initialize(h_), "mhpc_initialize");
    refresh_phases(false);
  }

  void solve_mhpc() {  // (:167-195)
    status_.assign(batch_, 0);
    check(mhpc_solve(h_, status_.data()), "mhpc_solve");
    refresh_phases(true);
  }

  // extension: which problem of the batch _phases, _actual_cost, _exp_cost_change and
  // _tconstr_violation describe (default 0; the reference holds exactly one problem)
  void select_problem(int b) {
    if (b < 0 || b >= batch_) throw std::runtime_error("select_problem: no such problem");
    problem_ = b;
    if (!pdesc_.empty()) desc_ = pdesc_[b];
    refresh_phases(solved_);
  }

  // MHPCLocomotion::print_debugInfo (MHPCLocomotion.cpp:293-380) for one problem:
  // state.txt, control.txt, gradient.txt, cost.txt in Eigen's default row format, with the
  // reference's row counts -- including its N_TIMESTEPS[i+2] for the SRB phases of
  // control / gradient / cost (exact for n_wbphase = 2; rows past an SRB phase's own N are
  // the zero-initialised buffer; clamped where the reference would read past the array).
  void print_debugInfo(int problem = 0) {
    const mhpc_problem_desc dsc = pdesc_.empty() ? desc_ : pdesc_[problem];
    const int nwb = dsc.n_wb, nfb = dsc.n_fb, np = nwb + nfb;
    struct Part { int n, N; std::vector<double> x, u, g, lx, phix; };
    std::vector<Part> parts(np);
    for (int p = 0; p < np; ++p) {
      Part& q = parts[p];
      check(mhpc_phase_dims(&dsc, p, &q.n, &q.N), "mhpc_phase_dims");
      q.x.resize((size_t)q.N * q.n); q.u.resize((size_t)q.N * 4); q.g.resize((size_t)q.N * q.n);
      q.lx.resize((size_t)(q.N - 1) * q.n); q.phix.resize(q.n);
      check(mhpc_get_phase_problems(h_, p, problem, 1, q.x.data(), q.u.data(), nullptr, nullptr,
                                    nullptr, q.g.data()), "mhpc_get_phase_problems");
      check(mhpc_get_cost_gradients_problems(h_, p, problem, 1, q.lx.data(), q.phix.data()),
            "mhpc_get_cost_gradients_problems");
    }
    auto n_rows = [&](int i) { return i + 2 < np ? parts[i + 2].N : parts[nwb + i].N; };
    // rows k < want of a [N][w] block, zero rows past N
    auto block = [](std::ofstream& f, const std::vector<double>& a, int N, int w, int want) {
      const std::vector<double> zero(w, 0.0);
      for (int k = 0; k < want; ++k) write_row(f, k < N ? &a[(size_t)k * w] : zero.data(), w);
    };
    std::ofstream gradient_output("gradient.txt"), state_output("state.txt"),
        contrl_output("control.txt"), cost_output("cost.txt");
    std::printf("********** Write to file state.txt ************\n");
    for (int i = 0; i < nwb; ++i) block(state_output, parts[i].x, parts[i].N, 14, parts[i].N);
    for (int i = 0; i < nfb; ++i) {
      const Part& q = parts[nwb + i];
      block(state_output, q.x, q.N, 6, q.N);
    }
    std::printf("********** Write to file control.txt ************\n");
    for (int i = 0; i < nwb; ++i) block(contrl_output, parts[i].u, parts[i].N, 4, parts[i].N);
    for (int i = 0; i < nfb; ++i) block(contrl_output, parts[nwb + i].u, parts[nwb + i].N, 4, n_rows(i));
    std::printf("********** Write to file gradient.txt ************\n");
    for (int i = 0; i < nwb; ++i) block(gradient_output, parts[i].g, parts[i].N, 14, parts[i].N);
    for (int i = 0; i < nfb; ++i) block(gradient_output, parts[nwb + i].g, parts[nwb + i].N, 6, n_rows(i));
    std::printf("********** Write to file cost.txt ************\n");
    for (int i = 0; i < nwb; ++i) {
      block(cost_output, parts[i].lx, parts[i].N - 1, 14, parts[i].N - 1);
      write_row(cost_output, parts[i].phix.data(), 14);
    }
    for (int i = 0; i < nfb; ++i) {
      const Part& q = parts[nwb + i];
      block(cost_output, q.lx, q.N - 1, 6, n_rows(i) - 1);
      write_row(cost_output, q.phix.data(), 6);
    }
  }

  // extension: the weights / constraint parameters the reference's WBCost, FBCost and
  // WBConstraint objects hold (MHPCCost.cpp:24-75, MHPCConstraints.cpp:14-88), replaceable
  // here for every later solve (mhpc_set_cost_weights / mhpc_set_constraint_params)
  void set_cost_weights(const mhpc_cost_weights& w) {
    check(mhpc_set_cost_weights(h_, &w), "mhpc_set_cost_weights");
  }
  mhpc_cost_weights get_cost_weights() {
    mhpc_cost_weights w{};
    check(mhpc_get_cost_weights(h_, &w), "mhpc_get_cost_weights");
    return w;
  }
  void set_constraint_params(const mhpc_constraint_params& c) {
    check(mhpc_set_constraint_params(h_, &c), "mhpc_set_constraint_params");
  }
  mhpc_constraint_params get_constraint_params() {
    mhpc_constraint_params c{};
    check(mhpc_get_constraint_params(h_, &c), "mhpc_get_constraint_params");
    return c;
  }
  // extension: the batch axis over weights and constraint parameters (one WBCost / FBCost /
  // WBConstraint set per controller in the reference).  Problem b solves with
  // weights[set_of_problem[b]] and constraints[set_of_problem[b]] (b % n_sets when empty); an
  // empty weights / constraints keeps problem 0's current values for that half.  Takes effect
  // at the next initialization() / update_problem(s) (mhpc_set_param_sets).
  void set_param_sets(const std::vector<mhpc_cost_weights>& weights,
                      const std::vector<mhpc_constraint_params>& constraints,
                      const std::vector<int32_t>& set_of_problem = {}) {
    if (weights.empty() && constraints.empty())
      throw std::runtime_error("set_param_sets: give weights, constraints or both");
    if (!weights.empty() && !constraints.empty() && weights.size() != constraints.size())
      throw std::runtime_error("set_param_sets: one weights and one constraints entry per set");
    if (!set_of_problem.empty() && (int)set_of_problem.size() != batch_)
      throw std::runtime_error("set_param_sets: one set index per problem expected");
    const int n = (int)(weights.empty() ? constraints.size() : weights.size());
    check(mhpc_set_param_sets(h_, n, weights.empty() ? nullptr : weights.data(),
                              constraints.empty() ? nullptr : constraints.data(),
                              set_of_problem.empty() ? nullptr : set_of_problem.data()),
          "mhpc_set_param_sets");
  }
  void get_problem_params(int b, mhpc_cost_weights* w, mhpc_constraint_params* c) {
    check(mhpc_get_problem_params(h_, b, w, c), "mhpc_get_problem_params");
  }
  int num_param_sets() {
    int n = 0;
    check(mhpc_num_param_sets(h_, &n), "mhpc_num_param_sets");
    return n;
  }

  // extension: per-problem option sets -- every controller of the reference owns its
  // MultiPhaseDDP::_option.  set_options: `_option = o` on every controller; set_option_sets:
  // problem b gets options[set_of_problem[b]] (b % n for an empty vector), 1..MHPC_MAX_OPTION_SETS
  // records that share the constructor's alpha.  Allowed at any point of the call order; the next
  // solve or tick reads the new records, and its launch schedule runs to the largest budgets among
  // the problems it covers (mhpc_set_option_sets).
  void set_options(const HSDDP_OPTION<TH>& option) {
    const mhpc_hsddp_option o = option_to_c(option);
    check(mhpc_set_options(h_, &o), "mhpc_set_options");
    _option = option;
  }
  HSDDP_OPTION<TH> get_options() { return get_problem_options(0); }
  void set_option_sets(const std::vector<HSDDP_OPTION<TH>>& options,
                       const std::vector<int32_t>& set_of_problem = {}) {
    if (!set_of_problem.empty() && (int)set_of_problem.size() != batch_)
      throw std::runtime_error("set_option_sets: one set index per problem expected");
    std::vector<mhpc_hsddp_option> os;
    for (const HSDDP_OPTION<TH>& o : options) os.push_back(option_to_c(o));
    check(mhpc_set_option_sets(h_, (int)os.size(), os.data(),
                               set_of_problem.empty() ? nullptr : set_of_problem.data()),
          "mhpc_set_option_sets");
    _option = get_options();
  }
  HSDDP_OPTION<TH> get_problem_options(int b) {
    mhpc_hsddp_option o;
    check(mhpc_get_problem_options(h_, b, &o), "mhpc_get_problem_options");
    return option_from_c(o);
  }
  int num_option_sets() {
    int n = 0;
    check(mhpc_num_option_sets(h_, &n), "mhpc_num_option_sets");
    return n;
  }

  const std::vector<int32_t>& status() const { return status_; }
  const mhpc_problem_desc& desc() const { return desc_; }
  mhpc_handle* handle() { return h_; }

  TH _actual_cost = 0, _exp_cost_change = 0, _tconstr_violation = 0;
  // MultiPhaseDDP's public phase list: _phases[p]->_V, _dV, _N_TIMESTEPS, get_nominal_ms_ptr()...
  std::vector<SinglePhaseAbstract<TH>*> _phases;
  int _n_phases = 0;
  HSDDP_OPTION<TH> _option;

 private:
  // from_snapshot: a fleet of a given descriptor and option record
  MHPCLocomotion(const mhpc_problem_desc& desc, const mhpc_hsddp_option& opt, Gait* gait, int batch,
                 int device)
      : batch_(batch), desc_(desc), opt_(opt) {
    check(mhpc_create(&desc_, &opt_, batch_, device, &h_), "mhpc_create");
    _option = option_from_c(opt_);
    _n_phases = desc_.n_wb + desc_.n_fb;
    gait_ = gait->to_c();
    xw_ = desc_.n_wb > 0 ? 14 : 6;
    pmax_ = _n_phases;
    refresh_phases(false);
    default_x0();
  }
  // every problem's layout (kept only when they differ), the x0 row width, the widest
  // phase count (the row width of mhpc_get_scalars' per-phase arrays)
  void refresh_descs() {
    std::vector<mhpc_problem_desc> ds(batch_);
    bool mixed = false;
    for (int b = 0; b < batch_; ++b) {
      ds[b] = problem_desc(b);
      mixed = mixed || std::memcmp(&ds[b], &ds[0], sizeof(mhpc_problem_desc)) != 0;
    }
    xw_ = 6;
    for (const mhpc_problem_desc& d : ds)
      if (d.n_wb > 0) xw_ = 14;
    check(mhpc_max_phases(h_, &pmax_), "mhpc_max_phases");
    desc_ = ds[problem_];
    pdesc_ = mixed ? std::move(ds) : std::vector<mhpc_problem_desc>();
    refresh_phases(false);
  }
  // the reference's default initial condition (MHPCLocomotion.cpp:37-39), projected for a
  // batch without whole-body phases
  // the host copy of x0 to the device, unless the device rows are the current ones
  // (set_x0_device, advance_x0)
  void push_x0() {
    if (!x0_on_device_) check(mhpc_set_x0(h_, x0_.data()), "mhpc_set_x0");
  }
  void default_x0() {
    x0_on_device_ = false;
    const double x0[14] = {0.0927, -0.1093, -0.1542, 1.0957, -2.2033, 0.9742, -1.7098,
                           0.9011, 0.2756,  0.7333,  0.0446, 0.0009,  1.3219, 2.7346};
    const int proj[6] = {0, 1, 2, 7, 8, 9};
    x0_.resize((size_t)batch_ * xw_);
    for (int b = 0; b < batch_; ++b)
      for (int i = 0; i < xw_; ++i) x0_[(size_t)b * xw_ + i] = xw_ == 14 ? x0[i] : x0[proj[i]];
  }
  // phase configuration from the selected problem's current layout; costs from the last solve
  void refresh_phases(bool scalars) {
    const int np = desc_.n_wb + desc_.n_fb;
    while ((int)phase_store_.size() < np) phase_store_.emplace_back(new SinglePhaseAbstract<TH>());
    _phases.clear();
    for (int p = 0; p < np; ++p) _phases.push_back(phase_store_[p].get());
    _n_phases = np;
    const size_t pw = (size_t)pmax_;
    std::vector<double> J(batch_), dV(batch_), viol(batch_), Vp((size_t)batch_ * pw),
        dVp((size_t)batch_ * pw);
    if (scalars)
      check(mhpc_get_scalars(h_, J.data(), dV.data(), viol.data(), Vp.data(), dVp.data(), nullptr),
            "mhpc_get_scalars");
    solved_ = scalars;
    for (int p = 0; p < np; ++p) {
      SinglePhaseAbstract<TH>& q = *_phases[p];
      q.h_ = h_;
      q.phase_ = p;
      q.problem_ = problem_;
      q.stale_ = true;
      q._modeidx = desc_.mode_seq[p];
      q._phaseidx = p;
      q._dt = p < desc_.n_wb ? desc_.dt_wb : desc_.dt_fb;
      q._N_TIMESTEPS = desc_.N[p];
      q._xsize = p < desc_.n_wb ? 14 : 6;
      q._V = scalars ? (TH)Vp[(size_t)problem_ * pw + p] : TH(0);
      q._dV = scalars ? (TH)dVp[(size_t)problem_ * pw + p] : TH(0);
    }
    if (scalars) {
      _actual_cost = J[problem_];
      _exp_cost_change = dV[problem_];
      _tconstr_violation = viol[problem_];
    }
  }
  static void check(int rc, const char* what) {
    if (rc != MHPC_OK)
      throw std::runtime_error(std::string(what) + ": " + mhpc_last_error());
  }
  // `ostream << vec.transpose()` with Eigen's default IOFormat: every coefficient printed
  // like `ostream << double` (%g, 6 significant digits), right-aligned to the widest
  // coefficient of the row, one space between coefficients
  static void write_row(std::ofstream& f, const double* v, int n) {
    std::vector<std::string> s(n);
    size_t w = 0;
    char buf[40];
    for (int i = 0; i < n; ++i) {
      std::snprintf(buf, sizeof buf, "%g", v[i]);
      s[i] = buf;
      if (s[i].size() > w) w = s[i].size();
    }
    for (int i = 0; i < n; ++i) {
      if (i) f << ' ';
      f << std::string(w - s[i].size(), ' ') << s[i];
    }
    f << '\n';
  }

  int batch_;
  mhpc_gait gait_{};
  mhpc_problem_desc desc_;
  mhpc_hsddp_option opt_;
  mhpc_handle* h_ = nullptr;
  std::vector<double> x0_;
  bool x0_on_device_ = false;
  std::vector<int32_t> status_;
  std::vector<std::unique_ptr<SinglePhaseAbstract<TH>>> phase_store_;
  std::vector<mhpc_problem_desc> pdesc_;  // per-problem layouts (empty: all equal desc_)
  int xw_ = 14, pmax_ = 0;
  int problem_ = 0;
  bool solved_ = false;
};
