/* mhpc_capi.h -- C-ABI boundary of the MI355X-native HSDDP solve path.
 *
 * Drop-in for the solve path that the reference runs under
 * MHPCLocomotion<double>::solve_mhpc() (Controller/MHPCLocomotion/MHPCLocomotion.cpp:167-195
 * -> HSDDPSolver/source/MultiPhaseDDP.cpp:154-289).  Plain C types only: pointers, sizes,
 * POD structs; no exceptions cross the ABI; every entry point returns an mhpc_status
 * (0 = OK).  One handle owns the device-resident state of a BATCH of independent MPC
 * problems; each problem has its own phase layout (gait schedule) drawn from a table of up to
 * MHPC_MAX_LAYOUTS distinct layouts (mhpc_set_layouts; by default every problem has the
 * layout given at create).  Calls on one handle are serialised by the caller; different
 * handles (devices, streams) are independent.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   mhpc_create          MHPCLocomotion ctor + memory_alloc      (MHPCLocomotion.cpp:8-43,218-261)
 *   mhpc_set_x0          MultiPhaseDDP::set_initial_condition   (MultiPhaseDDP.h:24-25); the
 *                        reference overwrites _x0 with its private default in
 *                        initialization() (MHPCLocomotion.cpp:49) -- settable here so a batch can
 *                        carry random initial states
 *   mhpc_initialize      MHPCLocomotion::initialization         (MHPCLocomotion.cpp:47-53):
 *                        memory_reset + build_problem (ReferenceGen::generate_ref,
 *                        ReferenceGen.h:53-109) + warmstart (bounding_PDcontrol,
 *                        boundingPDControl.cpp:3-46)
 *   mhpc_solve           MHPCLocomotion::solve_mhpc / MultiPhaseDDP::solve
 *                        (MHPCLocomotion.cpp:167-195, MultiPhaseDDP.cpp:154-289)
 *   mhpc_get_phase       SinglePhase::get_nominal_ms_ptr / get_CTG_info_ptr
 *                        (SinglePhase.cpp:364-373; fields of ModelState / CostToGoStruct,
 *                        MHPC_CompoundTypes.h:7-22,88-145)
 *   mhpc_get_scalars     MultiPhaseDDP::_actual_cost / _exp_cost_change /
 *                        _tconstr_violation and SinglePhaseAbstract::_V/_dV
 *                        (MultiPhaseDDP.h:57-60, SinglePhaseAbstract.h:116-118)
 *   mhpc_destroy         MHPCLocomotion::~MHPCLocomotion / memory_free (MHPCLocomotion.cpp:383-470)
 *   mhpc_update_problem  MHPCLocomotion::update_problem          (MHPCLocomotion.cpp:107-158,
 *                        Gait.h:21-77): gait advance, phase-buffer rotation, re-init
 *   mhpc_set_layouts     one MHPCLocomotion per controller, each built from its own Gait
 *                        (MHPCLocomotion.cpp:63-104): per-problem phase layouts in one batch
 *   mhpc_update_problems update_problem of every controller with its own gait and step count
 *   mhpc_reset_problems  set_initial_condition + initialization() of single controllers of the
 *                        fleet (MHPCLocomotion.cpp:47-53): the listed problems only
 *   mhpc_copy_problems   copy construction / assignment of a controller object (every member of
 *                        MHPCLocomotion and its MultiPhaseDDP): problems copied between slots
 *   mhpc_snapshot_problems / mhpc_restore_problems   nothing: the reference's controller is an
 *                        object in one process.  Here the same copy, serialised: live problems to
 *                        a blob of plain bytes and back into any handle, in any process
 *                        (mhpc_snapshot_size, _info, _entry, _status read sizes and entries)
 *   mhpc_tick_problems   set_initial_condition + update_problem + solve_mhpc of single controllers
 *                        of the fleet (MHPCLocomotion.cpp:107-158,167-195), each when its own gait
 *                        mode ends: the listed problems only; mhpc_reserve_knots the room that
 *                        memory_alloc's N_TIMESTEPS_MAX buffers give every controller
 *   mhpc_set_commands    MHPCUserParameters::usrcmd of every controller (vel, height), which
 *                        build_problem / update_problem hand to ReferenceGen
 *                        (MHPCLocomotion.cpp:98-103): per-problem user commands in one batch;
 *                        mhpc_get_commands reads them back
 *   mhpc_set_option_sets MultiPhaseDDP::_option of every controller (MultiPhaseDDP.h,
 *                        MHPC_CompoundTypes.h:196-212): per-problem iteration budgets, thresholds
 *                        and AL / ReB switches in one batch; mhpc_set_options `_option = o` on every
 *                        controller, mhpc_get_options / mhpc_get_problem_options read them back
 *   mhpc_get_reference_problems  ReferenceGen::generate_ref's ms_ref_*[p][k].x
 *                        (ReferenceGen.h:53-109): the tracking reference the costs use
 *   mhpc_rollout_policy  set_initial_condition(x) + forward_sweep_dynamics_only(0)
 *                        (SinglePhase.cpp:117-144, chained over phases through phase_transition by
 *                        MultiPhaseDDP.cpp:56-76): the solved feedback policy run from a measured
 *                        state; mhpc_rollout_policy_phase its trajectories, mhpc_advance_x0 the
 *                        same as the next tick's set_initial_condition, mhpc_get_x0 reads _x0
 *   mhpc_control         one knot of forward_sweep_dynamics_only, u = u_nom + K (x - x_nom)
 *                        (SinglePhase.cpp:117-144), for every problem at a control step of its own;
 *                        mhpc_control_device the same on device arrays of the caller's,
 *                        mhpc_set_x0_device set_initial_condition from one (the reference has
 *                        neither: its controller is one object on one CPU)
 *   mhpc_export_plan_device   get_nominal_ms_ptr() / get_CTG_info_ptr() of the next control steps
 *                        (SinglePhase.h's per-knot x, u, y and K, du, G) of the listed problems, and
 *                        mhpc_export_results_device their _actual_cost, _exp_cost_change,
 *                        _tconstr_violation, _V, _dV, into device arrays of the caller's
 *   mhpc_import_plan_device   a write into _phases[p]->get_nominal_ms_ptr() / get_CTG_info_ptr()
 *                        between initialization() or update_problem() and solve_mhpc(): the
 *                        reference's own warmstart() does exactly that for the whole-body phases'
 *                        controls (MHPCLocomotion.cpp:47-53, 200-215), and MultiPhaseDDP::solve
 *                        starts with forward_sweep(0) (MultiPhaseDDP.cpp:187), a real rollout of
 *                        u = u_nom + 0 du + K (x - x_nom) from _x0 (SinglePhase.cpp:62-114, :76).
 *                        Here: the listed problems' u_nom (and K, x_nom) from device arrays of the
 *                        caller's, and their next first sweep the real rollout; mhpc_import_plan
 *                        the same from host arrays, mhpc_num_plan_steps counts the steps
 */
#ifndef MHPC_CAPI_H
#define MHPC_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHPC_MAX_PHASES 16
#define MHPC_MAX_KNOTS 1024
#define MHPC_MAX_LAYOUTS 32   /* distinct phase layouts (gait schedules) per handle */
#define MHPC_MAX_OPTION_SETS 32 /* distinct mhpc_hsddp_option records per handle */
#define MHPC_TRACE_LEN 64

typedef enum {
  MHPC_OK = 0,
  MHPC_ERR_INVALID = 1,  /* bad argument / descriptor */
  MHPC_ERR_DEVICE = 2,   /* HIP runtime error (message via mhpc_last_error) */
  MHPC_ERR_STATE = 3     /* call order violated (e.g. solve before initialize) */
} mhpc_status;

/* Per-problem solve outcome (status array of mhpc_solve). */
typedef enum {
  MHPC_SOLVE_OK = 0,          /* finished all AL iterations or met AL_thresh */
  MHPC_SOLVE_REG_ABORT = 1,   /* regularization > 1000: early return (MultiPhaseDDP.cpp:218-226) */
  MHPC_SOLVE_NONFINITE = 2    /* non-finite total cost at the end of the solve */
} mhpc_solve_status;

/* Phase layout. As in MHPCLocomotion::build_problem (MHPCLocomotion.cpp:63-104) the n_wb
 * whole-body phases come first, then n_fb single-rigid-body phases; mode_seq[p] in 1..4
 * (1 back stance, 2 flight, 3 front stance, 4 flight); N[p] knots per phase.  dt values
 * are the reference's float parameters promoted to double.
 * n_wb == 0 is accepted (SRB-only problems, config C1). */
typedef struct {
  int32_t n_wb;
  int32_t n_fb;
  int32_t mode_seq[MHPC_MAX_PHASES];
  int32_t N[MHPC_MAX_PHASES];
  double dt_wb;
  double dt_fb;
  double vel_cmd;     /* USRCMD::vel (float promoted) */
  double height_cmd;  /* USRCMD::height */
  int32_t precision;  /* 64: fp64 (the reference's MHPCLocomotion<double>); 32: the fp32
                       * instantiation of the same kernels (config C5).  Host arrays at
                       * the ABI stay double in both cases. */
  int32_t reserved;
} mhpc_problem_desc;

/* Field-for-field HSDDP_OPTION<double> (MHPC_CompoundTypes.h:196-212). */
typedef struct {
  double alpha;
  double gamma;
  double update_penalty;
  double update_relax;
  double update_regularization;
  double update_ReB;
  double max_DDP_iter;
  double max_AL_iter;
  double DDP_thresh;
  double AL_thresh;
  int32_t AL_active;
  int32_t ReB_active;
  int32_t smooth_active;
  int32_t reserved;
} mhpc_hsddp_option;

/* Aggregate counters of the last mhpc_solve (sums over the batch). */
typedef struct {
  int64_t ddp_iters;        /* inner DDP iterations executed */
  int64_t bws_sweeps;       /* backward sweeps incl. failed (retried) ones */
  int64_t bws_knots;        /* knots swept backward (incl. partial failed sweeps) */
  int64_t ls_rollouts;      /* line-search rollouts the serial reference would run */
  int64_t fwd_sweeps;       /* full forward sweeps (forward_sweep(0)) */
  int64_t partial_sweeps;   /* forward_sweep_partials_only calls */
  double solve_ms;          /* device time of the last solve (HIP events) */
} mhpc_counters;

typedef struct mhpc_handle mhpc_handle;

/* Library identification / diagnostics. */
const char* mhpc_version(void);
const char* mhpc_last_error(void);

/* Number of knots/entries helpers for sizing caller buffers. */
int mhpc_phase_dims(const mhpc_problem_desc* desc, int phase, int* xsize, int* N);

int mhpc_create(const mhpc_problem_desc* desc, const mhpc_hsddp_option* opt, int batch,
                int device, mhpc_handle** out);
/* x0: [batch][xsize of phase 0] row-major host array. */
int mhpc_set_x0(mhpc_handle* h, const double* x0);
int mhpc_initialize(mhpc_handle* h);
/* status: optional host array [batch] of mhpc_solve_status. */
int mhpc_solve(mhpc_handle* h, int32_t* status);
/* Copy out the nominal solution of one phase; any pointer may be NULL.
 * Shapes (row-major, host): x [batch][N][xsize], u/y/du [batch][N][4],
 * K [batch][N][4][xsize], Vx [batch][N][xsize]. */
int mhpc_get_phase(mhpc_handle* h, int phase, double* x, double* u, double* y, double* K,
                   double* du, double* Vx);
/* mhpc_get_phase for problems [first, first + count) of the batch only (shapes with
 * count in place of batch): one problem's phase, as the reference's single-problem
 * _phases[p]->get_nominal_ms_ptr() / get_CTG_info_ptr() hold it (SinglePhaseAbstract.h:79-81). */
int mhpc_get_phase_problems(mhpc_handle* h, int phase, int first, int count, double* x, double* u,
                            double* y, double* K, double* du, double* Vx);
/* J, dV_exp, viol: [batch]; V_phase, dV_phase: [batch][P] with P = mhpc_max_phases (the
 * largest phase count over the problems' layouts -- not mhpc_get_desc's n_wb + n_fb, which is
 * problem 0's; entries past a problem's own phases are zero); trace: [batch][MHPC_TRACE_LEN]
 * (decision trace, encoding in DESIGN.md §Parity); any pointer may be NULL. */
int mhpc_get_scalars(mhpc_handle* h, double* J, double* dV_exp, double* viol, double* V_phase,
                     double* dV_phase, int32_t* trace);
int mhpc_get_counters(mhpc_handle* h, mhpc_counters* c);

/* Gait schedule (the reference's Gait class, Common/header/Gait.h:14-77): the mode cycle and
 * the duration of every mode (timings[m-1], float as in the reference). */
typedef struct {
  int n_modes;
  int modes[MHPC_MAX_PHASES];
  float timings[MHPC_MAX_PHASES];
} mhpc_gait;

/* MHPCLocomotion::update_problem (MHPCLocomotion.cpp:107-158), whole batch: advance the gait
 * by one mode, rotate the WB / SRB phase buffers by one (the solution just computed becomes
 * the warm start of the shifted horizon), recompute mode sequence and knot counts
 * (round(timing / dt)), regenerate the references from the current x0 (set it first with
 * mhpc_set_x0 -- the reference's set_initial_condition) and re-initialise the AL / ReB
 * parameters.  Then call mhpc_solve again.  The phase descriptor reported by
 * mhpc_get_desc changes accordingly. */
int mhpc_update_problem(mhpc_handle* h, const mhpc_gait* gait);
/* The handle's current phase layout (changes with mhpc_update_problem); with per-problem
 * layouts (mhpc_set_layouts) the layout of problem 0. */
int mhpc_get_desc(mhpc_handle* h, mhpc_problem_desc* desc);

/* ---- per-problem phase layouts: the batch axis over gait schedules --------------------
 * In the reference every controller instance builds its phase layout from its own Gait and
 * gait point (MHPCLocomotion::build_problem, MHPCLocomotion.cpp:63-104; Gait.h:21-77) and
 * rotates it per control tick (update_problem, :107-158).  A handle starts with the
 * descriptor of mhpc_create for every problem; mhpc_set_layouts gives problem b the
 * descriptor descs[layout_of_problem[b]] (1 <= n_desc <= MHPC_MAX_LAYOUTS; precision,
 * vel_cmd and height_cmd must equal the handle's; NULL layout_of_problem: descs[b % n_desc]).
 * The arrays grow when a layout has more knots than any before.  The handle is then
 * uninitialised: mhpc_set_x0 (rows of 14 when any layout has a whole-body phase -- an
 * SRB-only problem reads the first 6 of its row -- else 6) and mhpc_initialize precede the
 * next solve.  Problems sharing a layout are solved together, a launch never mixes layouts
 * inside a block, and each problem's arithmetic is the one it gets in a handle of its own
 * layout, bit for bit (tests/test_gpu_layouts.py).  Outputs: mhpc_get_phase_problems needs
 * a problem range whose phase has one shape (knots, state size); mhpc_get_scalars' V_phase /
 * dV_phase rows are max-phase-count long, zero past a problem's phases. */
int mhpc_set_layouts(mhpc_handle* h, int n_desc, const mhpc_problem_desc* descs,
                     const int32_t* layout_of_problem);
/* The current phase layout of problem b (changes with mhpc_update_problem[s]). */
int mhpc_get_problem_desc(mhpc_handle* h, int problem, mhpc_problem_desc* desc);
/* Per-problem MHPCLocomotion::update_problem: problem b takes steps[b] >= 0 gait steps of
 * gaits[gait_of_problem[b]] (one step = one update_problem: the WB / SRB phase buffers
 * rotate by one, the next mode starts the horizon, knot counts round(timing / dt)); with
 * steps[b] = 0 it keeps its layout and warm start.  Every problem's references are then
 * regenerated from its current x0 and its AL / ReB parameters re-initialised, as
 * update_problem does, and the next mhpc_solve starts from the (rotated) solutions.
 * NULL gait_of_problem: gaits[0] for every problem; NULL steps: one step each (then this is
 * mhpc_update_problem).  n_gaits in 1..MHPC_MAX_LAYOUTS. */
int mhpc_update_problems(mhpc_handle* h, int n_gaits, const mhpc_gait* gaits,
                         const int32_t* gait_of_problem, const int32_t* steps);
/* ---- per-problem re-initialisation: restart lost problems inside a live batch -----------
 * MHPCLocomotion::initialization() (MHPCLocomotion.cpp:47-53: memory_reset, build_problem,
 * ReferenceGen::generate_ref, warmstart) for the n listed problems only: a fleet restarts one
 * controller with set_initial_condition + initialization() on that object, and the others
 * never notice.  problems: n distinct problem numbers, 1 <= n <= batch.  x0: [n][r] rows in
 * list order (r as in mhpc_set_x0); NULL keeps each listed problem's current device row (a
 * fresh warm start from where the robot is).  descs == NULL (n_desc == 0): each listed problem
 * keeps its current descriptor, its phase buffers go back to identity and its gait to the
 * descriptor's first mode, as mhpc_initialize does.  descs != NULL: listed problem i gets
 * descs[desc_of ? desc_of[i] : i % n_desc] (mhpc_set_layouts' checks; the handle's x0 row width
 * must not change).
 *  - A listed problem comes out as mhpc_initialize leaves a problem: x0 row, position
 *    references, solver state (status, trace, counters, the option values a solve rewrites),
 *    the AL / ReB initial values of its own parameter set, the PD warm start, zero K / du / G,
 *    zero phase buffers.  Its command and parameter set belong to the problem number and stay.
 *  - Every other problem's device state stays bit for bit.  So a reset never changes the knot
 *    stride and never reallocates: MHPC_ERR_INVALID, before anything changes, for a descriptor
 *    with more knots than the current stride, or -- once the phase-buffer store exists (after the
 *    first mhpc_update_problem[s]) -- more phases or a longer phase than the store holds; also for
 *    duplicate or out-of-range problem numbers and for more than MHPC_MAX_LAYOUTS groups.  The
 *    stride stays even when the longest problem leaves its layout (a later
 *    mhpc_update_problem[s] may shrink it).
 *  - MHPC_ERR_STATE before mhpc_initialize.  The call-order state of the handle (solved, pending
 *    x0 / commands / parameters) stays as it is.  Both orders work: mhpc_solve ->
 *    mhpc_reset_problems -> mhpc_update_problems with steps[b] = 0 for the reset problems ->
 *    mhpc_solve; and mhpc_initialize / mhpc_update_problem[s] -> mhpc_reset_problems -> mhpc_solve.
 *    Either way the reset problems' next solve is the one of a freshly initialised handle, bit for
 *    bit (tests/test_gpu_reset.py).
 *  - Device work is proportional to n, not to the batch. */
int mhpc_reset_problems(mhpc_handle* h, int n, const int32_t* problems, const double* x0,
                        int n_desc, const mhpc_problem_desc* descs, const int32_t* desc_of);
/* ---- per-problem ticks: update and solve the listed problems, and nobody else -------------
 * In the reference every robot is its own MHPCLocomotion and ticks when its own gait mode ends:
 * set_initial_condition(x), update_problem() (MHPCLocomotion.cpp:107-158), solve_mhpc()
 * (:167-195); the other robots never notice.  One MPC tick of the n listed problems: for listed
 * problem i its x0 row, steps[i] update_problem steps of gaits[gait_of[i]], then the solve.
 * problems: n distinct problem numbers, 1 <= n <= batch, in any order.  x0: [n][r] rows in list
 * order (r as in mhpc_set_x0; an SRB-only problem reads its first 6 entries), finite; NULL keeps
 * each listed problem's current device row (what mhpc_set_x0_device or mhpc_advance_x0 left
 * there).  gait_of: [n], NULL = gaits[0]; n_gaits in 1..MHPC_MAX_LAYOUTS.  steps: [n], each in
 * 0..1024, NULL = one step each; with steps[i] = 0 the problem keeps its layout and is re-solved
 * from its new x0 (what mhpc_update_problems does for such a problem); gaits may be NULL only when
 * every step is 0.  status: optional, [n] in list order (mhpc_solve_status).  ms: optional, device
 * time of the whole tick (HIP events).
 *  - A listed problem is afterwards, bit for bit, what it would be after mhpc_set_x0 of that row,
 *    mhpc_update_problems with those steps and mhpc_solve in a handle of its own with the same
 *    descriptor history, command, parameter set and options: the nominal trajectory and every
 *    slot, K / du / G, the partials, impact Jacobians and sweep carry, the whole solver state, the
 *    position references (generated from the problem's current command), the layout with its
 *    rotated buffers and gait point, its rows of the phase-buffer store -- in fp64 and in fp32
 *    (tests/test_gpu_tick.py).  For a problem that mhpc_reset_problems made fresh and that takes 0
 *    steps the first forward_sweep(0) is the cost evaluation, as in mhpc_solve.
 *  - Every unlisted problem keeps its device state bit for bit: every array above, its x0 row, its
 *    store rows.  So a tick never re-strides or reallocates: a listed problem whose new layout has
 *    more knots than the current stride, or a phase longer than the phase buffers, is refused
 *    before anything changes (mhpc_reserve_knots makes room beforehand).  The first tick or update
 *    after an mhpc_initialize still zeroes the phase-buffer store once: the only batch-proportional
 *    device work.
 *  - MHPC_ERR_STATE unless the handle is initialised and its last batch-wide step was a solve, and
 *    while constraint parameters or parameter sets are pending.  A pending x0 does not block the
 *    call and stays pending.  Pending commands do not block it either: the tick applies the listed
 *    problems' current commands and clears their part of the pending state (commands are pending
 *    per problem: mhpc_set_commands marks the problems whose value changed, mhpc_initialize /
 *    mhpc_update_problem[s] clear every mark, a tick the listed ones; the other entry points
 *    refuse while any problem is marked).  The call-order state is otherwise unchanged: solved.
 *  - mhpc_get_counters (solve_ms included) and the per-kernel byte / flop accounting afterwards
 *    describe the tick's solve: sums over the listed problems.
 *  - MHPC_ERR_INVALID, before anything is launched or changed: a null required pointer; n out of
 *    range; a duplicate or out-of-range problem; a bad gait or gait index; a step count out of
 *    range; a non-finite x0 entry; a current mode that is not in the gait, a phase with N < 2 or
 *    too many knots (mhpc_update_problems' refusals); a layout that does not fit the arrays; more
 *    than MHPC_MAX_LAYOUTS groups.  A refused call changes nothing.
 *  - MHPC_ERR_DEVICE: a failed launch leaves the listed problems undefined, as a failed
 *    mhpc_reset_problems does (reset them).
 *  - Device work is proportional to n, not to the batch.  The host plan and the group-table upload
 *    stay O(batch), as for a reset; when every step is 0 no layout changes and both are skipped. */
int mhpc_tick_problems(mhpc_handle* h, int n, const int32_t* problems, const double* x0,
                       int n_gaits, const mhpc_gait* gaits, const int32_t* gait_of,
                       const int32_t* steps, int32_t* status, float* ms);
/* Floor of the per-problem knot stride of the packed arrays, knots in 1..MHPC_MAX_KNOTS: from
 * this call on the stride is max(longest layout, knots) wherever it may change, so a fleet created
 * at one gait point can later tick into a longer layout (1 WB + 2 SRB phases of the default gait:
 * 260 knots at mode 1, 280 at mode 2).  After mhpc_create / mhpc_set_layouts and before
 * mhpc_initialize: MHPC_ERR_STATE on an initialised handle.  Results do not depend on the stride. */
int mhpc_reserve_knots(mhpc_handle* h, int knots);
/* ---- copies of live problems: a slot becomes another controller, warm start and all -------
 * In the reference a controller is an object and copying it is copying the object.  Here dst
 * problem dst_problems[i] becomes a copy of src problem src_problems[i], i < n, as the source
 * stands at this call; dst == src copies inside one handle.  ms optional: device time of the copy
 * launch (HIP events), as mhpc_rollout_costs reports its own.
 *  - What travels: the nominal trajectory and every line-search slot, K / du / G, the partials
 *    records and impact Jacobians, the solver state (status, trace, counters, AL / ReB values, the
 *    option values a solve rewrites), the x0 row on the device, the position references, the
 *    layout with its phase-buffer rotation and gait point, the problem's rows of the phase-buffer
 *    store -- and, unlike mhpc_reset_problems, the command, the parameter set and the option set: a
 *    clone that kept the destination's would not be a clone (the source's parameter set joins dst's
 *    sets under mhpc_set_param_sets' merge rules; change either afterwards with the setters).  The
 *    option set travels as an index: inside one handle the destination takes the source's; between
 *    handles the source problem's record (every field) must already be one of dst's option sets
 *    (mhpc_set_option_sets) -- the copy never adds a record to dst's table, so it never changes
 *    dst's launch schedule.  After the call
 *    every getter reports for the destination what it reports for the source, and every later
 *    mhpc_solve / mhpc_update_problem(s) / mhpc_advance_x0 of the destination equals the source's
 *    under the same inputs, bit for bit, in both precisions (tests/test_gpu_copy.py).
 *  - Every unlisted problem of dst and every problem of src keeps its device state bit for bit.
 *    The copy never re-strides or reallocates dst's packed arrays: it copies the knots below the
 *    smaller of the two knot strides and leaves the rest of dst's stride as a reset leaves it.  If
 *    src has a phase-buffer store and dst none, dst gets its own (zeroed, as at its first
 *    mhpc_update_problem[s]) and then the rows; if dst has one and src none, the destination
 *    problems' rows are zeroed.
 *  - MHPC_ERR_INVALID, before anything changes: a null pointer; n < 1 or n > dst's batch; a
 *    problem number out of range; a destination listed twice (a source may repeat: one to many);
 *    with dst == src a number that is both a source and a destination; handles of different
 *    precision, device, alpha (the line-search grid) or backward-sweep arithmetic
 *    (MHPC_VARIANT_SWEEP_BITS 32 on one side only: the one kernel variant that changes results;
 *    every other variant computes the same bits and may differ); a source layout with more knots than
 *    dst's knot stride or -- once dst's store exists -- more phases or a longer phase than it holds;
 *    x0 rows of different width (14 vs 6); more than MHPC_MAX_LAYOUTS (layout, set) groups; a
 *    source problem whose option record is none of dst's (two handles whose options differ in any
 *    field have no common record).
 *  - MHPC_ERR_STATE: either handle before mhpc_initialize, or with commands, constraint parameters
 *    or parameter sets pending, or the two handles at different points of the call order (one just
 *    solved, the other just initialized or updated).  A pending x0 is allowed: the device's current
 *    row is what is copied.  The call-order state of both handles stays as it is.
 *  - MHPC_ERR_DEVICE: a failure before the copy launch is queued (allocating dst's store,
 *    uploading the lists) leaves both handles as they were; a failed launch leaves the destination
 *    problems undefined, as a failed mhpc_reset_problems does (reset or copy them again).
 *  - Device work is proportional to n, not to either batch. */
int mhpc_copy_problems(mhpc_handle* dst, const int32_t* dst_problems, mhpc_handle* src,
                       const int32_t* src_problems, int n, float* ms);
/* ---- snapshots of live problems: the batch axis over controller lifetimes across processes ----
 * mhpc_copy_problems ends at the process boundary: both handles alive, one process, one device.
 * A snapshot is the serialised form of the same object: the listed problems, as they stand at the
 * call, as plain bytes in a host buffer of the caller's (pageable or pinned) -- no pointers,
 * device indices or handle addresses in it --, to be written to a file, sent to another rank or
 * kept for a replay; mhpc_restore_problems makes problems of any handle that could have been the
 * destination of that copy (this one later, one in another process, on another device) become
 * entries of the blob.
 *  - Contract: a restore is the mhpc_copy_problems the caller could have made at the moment of
 *    the snapshot, had the source handle still been there.  Everything that travels with the copy
 *    travels (see above: every slot, K / du / G, partials, impact Jacobians, solver state, x0 row,
 *    references, layout with rotation and gait point, store rows, command, parameter set, option
 *    record, the ledger's per-problem marks).  Afterwards every getter reports for the destination
 *    what it reported for the source at the snapshot, every later mhpc_solve /
 *    mhpc_update_problem(s) / mhpc_tick_problems / mhpc_advance_x0 / mhpc_control of it equals the
 *    source's under the same inputs bit for bit in both precisions, every unlisted problem of the
 *    destination keeps its device state bit for bit, and the destination's arrays are never
 *    re-strided or reallocated (tests/test_gpu_snapshot.py).  The source keeps its device and host
 *    state bit for bit.
 *  - Blob: header | entry table | payload (mhpc_snapshot_map.h).  The payload's knot
 *    stride is the largest knot count among the listed problems' layouts, not the handle's: a
 *    robot taken out of a handle with a large mhpc_reserve_knots does not carry the reservation.
 *    Store rows travel with the source's store shape, or with none.  Two snapshots of the same
 *    unchanged problems are byte-identical.  MHPC_SNAPSHOT_VERSION names the format; a blob is
 *    read only by the version, precision and record sizes that wrote it.
 *  - mhpc_snapshot_size: the exact blob size for these problems.  mhpc_snapshot_problems: bytes
 *    must be at least that; exactly that many are written.  problems: n distinct numbers,
 *    1 <= n <= batch.  ms optional: device time of the pack launches (HIP events).
 *  - mhpc_snapshot_info / _entry / _status work on host memory alone: no handle, no GPU.  entry i's
 *    descriptor carries its command; option, weights, constraints are its records by value;
 *    mhpc_snapshot_status gives the mhpc_solve_status of entries [first, first + count) as their
 *    last solve left it (status [count], read from the solver state in the payload).  Any output pointer of mhpc_snapshot_entry may be NULL.  With them a caller sizes
 *    and configures a handle for the blob (MHPCLocomotion::from_snapshot does).
 *  - mhpc_restore_problems: destination problem dst_problems[i] becomes blob entry entries[i]
 *    (entries == NULL: entry i); an entry may repeat (one to many).  ms optional: device time of
 *    the unpack launches.
 *  - Refusals are the copy's, checked before anything changes, MHPC_ERR_INVALID: another
 *    precision, alpha / slot count, sweep arithmetic or x0 row width; a layout that does not fit
 *    the destination's knot stride or store; an option record that is none of the destination's;
 *    more than MHPC_MAX_LAYOUTS groups; a destination listed twice; an entry out of range.
 *    MHPC_ERR_STATE: the handle not initialised; commands or parameters pending (on the source at
 *    the snapshot, on the destination at the restore).
 *  - Call-order point: the blob records the source's (just initialised / updated / solved).  A
 *    restore that lists every problem of the destination makes the destination adopt it -- resume
 *    from a checkpoint into a handle that was only created and initialised.  A partial restore
 *    requires equal points, as the copy does (MHPC_ERR_STATE).
 *  - Blob validation, MHPC_ERR_INVALID with the cause in mhpc_last_error: a buffer too small or a
 *    length that does not match the header; a wrong magic; another format version; a build whose
 *    sizeof(ProbState), sizeof(BwsCarry), element size or record widths differ from the header's;
 *    a header / entry-table checksum mismatch.
 *  - Device work and staging memory are proportional to n, never to the batch.  A list whose
 *    payload exceeds the staging cap runs in rounds of R problems through two staging buffers on
 *    the handle's two streams: packing round i + 1 overlaps the device-to-host copy of round i,
 *    and the reverse for a restore.  mhpc_set_kernel_variant(h, MHPC_VARIANT_SNAP_ROUND, R) forces
 *    R.  After an error inside a round nothing more is queued and the handle's streams are
 *    drained; a failed restore leaves the destination problems undefined, as a failed copy does. */
#define MHPC_SNAPSHOT_VERSION 1
/* (a struct tag, not a typedef: the reader below has the same name, as stat has) */
struct mhpc_snapshot_info {
  int32_t version;        /* MHPC_SNAPSHOT_VERSION of the writer */
  int32_t n_entries;
  int32_t precision;      /* 64 / 32 */
  int32_t sweep_bits;     /* 64 / 32: arithmetic of the source's backward sweep */
  int32_t x0_row;         /* 14 / 6: the source's x0 row width */
  int32_t n_slots;        /* trajectory slots of the line-search grid (follows alpha) */
  int32_t knot_stride;    /* of the payload: the longest listed layout */
  int32_t store_knots;    /* store shape: knots a buffer, */
  int32_t store_buffers;  /*   buffers a problem (0: no store rows travel) */
  int32_t need_full;      /* the source's call-order point: next solve starts with a rollout, */
  int32_t solved;         /*   last batch-wide step was a solve */
  int32_t reserved;
  double alpha;
  int64_t payload_bytes_per_entry;
  int64_t total_bytes;
};
int mhpc_snapshot_size(mhpc_handle* h, int n, const int32_t* problems, int64_t* bytes);
int mhpc_snapshot_problems(mhpc_handle* h, int n, const int32_t* problems, void* blob,
                           int64_t bytes, float* ms);
int mhpc_snapshot_info(const void* blob, int64_t bytes, struct mhpc_snapshot_info* info);
int mhpc_restore_problems(mhpc_handle* h, int n, const int32_t* dst_problems, const void* blob,
                          int64_t bytes, const int32_t* entries, float* ms);
int mhpc_snapshot_status(const void* blob, int64_t bytes, int first, int count, int32_t* status);

/* ---- per-problem user commands: the batch axis over speed / height commands -----------
 * Per-problem user command (the reference's MHPCUserParameters::usrcmd of each controller,
 * MHPCLocomotion.cpp:98-103).  vel, height: host arrays [batch]; either may be NULL = unchanged.
 * A handle starts with vel_cmd / height_cmd of mhpc_create's descriptor for every problem.
 * Every entry must be finite (no sign or range restriction: the reference has none); the fp32
 * build rounds to float.  Commands belong to the problem number: they survive
 * mhpc_set_layouts and mhpc_update_problem(s), and mhpc_get_problem_desc(b) reports problem
 * b's (mhpc_get_desc: problem 0's).  New values take effect at the next mhpc_initialize or
 * mhpc_update_problem(s), which regenerate every problem's references; set on an initialized
 * handle they make mhpc_solve and mhpc_rollout_costs return MHPC_ERR_STATE until one of those
 * has run (the position references would otherwise belong to the old speed).  A call whose
 * values all equal the current ones changes nothing. */
int mhpc_set_commands(mhpc_handle* h, const double* vel, const double* height);
int mhpc_get_commands(mhpc_handle* h, double* vel, double* height);   /* either may be NULL */
/* The tracking reference x of `phase` for problems [first, first+count): [count][N][xsize],
 * the reference's ms_ref_*[p][k].x as ReferenceGen::generate_ref leaves it
 * (ReferenceGen.h:53-109).  The range's phase must have one shape (as mhpc_get_phase_problems). */
int mhpc_get_reference_problems(mhpc_handle* h, int phase, int first, int count, double* xref);

/* Distinct phase layouts currently in use (1 for a homogeneous batch). */
int mhpc_num_layouts(mhpc_handle* h, int* n);
/* The largest phase count over the problems' current layouts: the row length of
 * mhpc_get_scalars' V_phase / dV_phase. */
int mhpc_max_phases(mhpc_handle* h, int* n);

/* ---- cost and constraint parameters (the reference's downward plugin points) --------
 * The reference's solve reads its weights through CostAbstract / Cost<T,X,U,Y>
 * (HSDDPSolver/header/CostBase.h:9-46: diagonal _Q, _R, _S, _Qf per mode) and its
 * inequality / AL parameters through Constraint (ConstraintsBase.h:11-50: AL_REB_PARAMETER per
 * mode), with the values MHPCCost.cpp:24-75 and MHPCConstraints.cpp:14-88 set.  A handle
 * starts from those values; mhpc_set_* replaces them for every later solve (the kernels read
 * them from a device table, one record per group of problems).  Rows are modes 1..4. */
typedef struct {
  double wb_Q[4][14];  /* WBCost _Q diagonal (0.01 * q) */
  double wb_R[4][4];   /* WBCost _R diagonal (0.5 * r[m]) */
  double wb_S[4][4];   /* WBCost _S diagonal (s[m]; s[3] uninitialised in the reference: 0) */
  double wb_Qf[4][14]; /* WBCost _Qf diagonal (100 * qf[m]) */
  double fb_Q[4][6];   /* FBCost _Q diagonal (0.01 * q) */
  double fb_R[4][4];   /* FBCost _R diagonal (r[m]); FBCost _S is zero (SRB y == 0) */
  double fb_Qf[4][6];  /* FBCost _Qf diagonal (100 * qf) */
} mhpc_cost_weights;

typedef struct {
  double torque_limit;     /* WBConstraint b_torque: -limit <= u_i <= limit (33) */
  double friction_coeff;   /* WBConstraint _friccoeff of the GRF cone (0.5) */
  double sigma[4];         /* AL penalty at initialisation, modes with a touchdown
                              constraint (2, 4) only: 5 */
  double delta[4];         /* ReB relaxation at initialisation (0.1) */
  double delta_min[4];     /* its lower bound in the AL update (0.01) */
  double eps_torque[4];    /* ReB weight of the torque limits (0.01) */
  double eps_grf[4];       /* ReB weight of the GRF constraints, stance modes 1 / 3 (0.01) */
  /* The joint limits carry eps_ReB = 0 in the reference (MHPCConstraints.cpp:60-82) and
   * contribute exact zeros; they are not a parameter here. */
} mhpc_constraint_params;

/* The reference's values (MHPCCost.cpp:24-75, MHPCConstraints.cpp:14-88). */
int mhpc_default_cost_weights(mhpc_cost_weights* w);
int mhpc_default_constraint_params(mhpc_constraint_params* c);
/* Replace / read the handle's parameters; take effect from the next mhpc_initialize /
 * mhpc_update_problem (AL / ReB initial values) and mhpc_solve (weights, limits).  Every
 * entry must be finite, weights >= 0, torque_limit > 0, friction_coeff >= 0,
 * 0 < delta_min <= delta.  Constraint parameters set on an initialized handle make
 * mhpc_solve return MHPC_ERR_STATE until mhpc_initialize or mhpc_update_problem has applied
 * their initial values (a solve would otherwise run the new limits with the old AL / ReB
 * state). */
int mhpc_set_cost_weights(mhpc_handle* h, const mhpc_cost_weights* w);
int mhpc_get_cost_weights(mhpc_handle* h, mhpc_cost_weights* w);
int mhpc_set_constraint_params(mhpc_handle* h, const mhpc_constraint_params* c);
int mhpc_get_constraint_params(mhpc_handle* h, mhpc_constraint_params* c);
/* Entry `entry` of a snapshot blob (see "snapshots of live problems" above; host memory only):
 * its descriptor with its command, option record and parameter values; any of them may be NULL. */
int mhpc_snapshot_entry(const void* blob, int64_t bytes, int entry, mhpc_problem_desc* desc,
                        mhpc_hsddp_option* option, mhpc_cost_weights* weights,
                        mhpc_constraint_params* constraints);

/* ---- per-problem parameter sets: the batch axis over weights and constraint parameters --
 * In the reference every MHPCLocomotion owns its WBCost / FBCost / WBConstraint objects
 * (MHPCCost.cpp:24-75, MHPCConstraints.cpp:14-88), so a fleet of controllers is also a fleet of
 * weight and limit sets.  Problem b solves with weights w[set_of_problem[b]] and constraint
 * parameters c[set_of_problem[b]] (host arrays of n_sets entries, 1 <= n_sets <=
 * MHPC_MAX_PARAM_SETS).  w == NULL / c == NULL: every set keeps, for that half, the values
 * problem 0 has now.  set_of_problem == NULL: b % n_sets.  Every entry is validated as
 * mhpc_set_cost_weights / mhpc_set_constraint_params validate theirs; the fp32 build rounds to
 * float.  A handle starts with one set, the reference's values.
 *  - Sets belong to the problem number: they survive mhpc_set_layouts and
 *    mhpc_update_problem(s), as commands do.
 *  - Merging: after the conversion to the solve's arithmetic type, sets that compare equal are
 *    merged and sets no problem uses are dropped; mhpc_num_param_sets counts what is left.
 *  - mhpc_set_cost_weights / mhpc_set_constraint_params keep their meaning (every problem gets
 *    that value): after a mixed call one of them collapses that half of every set, so distinct
 *    sets may merge.  mhpc_get_cost_weights / mhpc_get_constraint_params report problem 0's
 *    values, as mhpc_get_desc does; mhpc_get_problem_params problem b's.
 *  - Problems sharing a layout and a set are solved together (a group): a launch never mixes
 *    groups inside a block, the group's parameters are read with scalar loads, and each
 *    problem's arithmetic is the one it gets in a handle of its own set through the handle-wide
 *    setters, bit for bit (tests/test_gpu_param_sets.py).  Distinct (layout, set) pairs in use
 *    are at most MHPC_MAX_LAYOUTS: mhpc_set_param_sets, mhpc_set_layouts and
 *    mhpc_update_problem(s) return MHPC_ERR_INVALID for a call that would exceed it.
 *    mhpc_num_layouts keeps counting distinct layouts.
 *  - New values take effect at the next mhpc_initialize / mhpc_update_problem(s) (AL / ReB
 *    initial values) and at the next solve (weights, limits).  Set on an initialized handle,
 *    mhpc_solve, mhpc_rollout_costs, the policy rollouts and mhpc_advance_x0 return
 *    MHPC_ERR_STATE until one of those has run, as after mhpc_set_constraint_params.  A call
 *    that changes no problem's values changes nothing and leaves nothing pending.
 *  - A refused call changes nothing. */
#define MHPC_MAX_PARAM_SETS 32
int mhpc_set_param_sets(mhpc_handle* h, int n_sets, const mhpc_cost_weights* w,
                        const mhpc_constraint_params* c, const int32_t* set_of_problem);
/* Problem b's current values; either pointer may be NULL. */
int mhpc_get_problem_params(mhpc_handle* h, int problem, mhpc_cost_weights* w,
                            mhpc_constraint_params* c);
/* Distinct sets in use (1 for a fresh handle). */
int mhpc_num_param_sets(mhpc_handle* h, int* n);

/* ---- per-problem option sets: the batch axis over iteration budgets and thresholds ---------
 * In the reference every MHPCLocomotion owns its MultiPhaseDDP::_option (MultiPhaseDDP.h,
 * MHPC_CompoundTypes.h:196-212), so a fleet of controllers is also a fleet of option values: a
 * robot just reset wants the full AL x DDP budget, the warm robots ticking beside it one AL
 * iteration and one or two DDP iterations.  Problem b solves with sets[set_of_problem[b]] (host
 * array of n_sets records, 1 <= n_sets <= MHPC_MAX_OPTION_SETS); set_of_problem == NULL:
 * b % n_sets.  mhpc_set_options gives every problem one record.  A handle starts with one set,
 * the option given to mhpc_create.
 *  - Sets belong to the problem number: they survive mhpc_set_layouts, mhpc_update_problem(s),
 *    mhpc_reset_problems and ticks, as commands and parameter sets do.
 *  - Merging: records that are equal in every field, bit for bit, are merged and records no
 *    problem uses are dropped; mhpc_num_option_sets counts what is left.  At most
 *    MHPC_MAX_OPTION_SETS distinct records may be in use: a call that would exceed it is
 *    MHPC_ERR_INVALID.  mhpc_get_options reports problem 0's record, mhpc_get_problem_options
 *    problem b's (the reserved field zero).
 *  - alpha stays handle-wide: it fixes the line-search grid and with it the trajectory slots and
 *    the arrays' shape.  A record whose alpha differs bitwise from the one given to mhpc_create
 *    is MHPC_ERR_INVALID.  Every other field is validated as mhpc_create validates it: every real
 *    field finite, iteration budgets at most 2^20.
 *  - Options are no grouping dimension: problems of different sets share launches, blocks and
 *    waves, and each reads its own record in its control flow.  They do not count against
 *    MHPC_MAX_LAYOUTS.  Each problem's arithmetic is the one it gets in a handle created with its
 *    record, bit for bit, in both precisions and every launch variant
 *    (tests/test_gpu_option_sets.py).
 *  - The launch schedule of a solve runs to the largest max_AL_iter and max_DDP_iter among the
 *    problems it covers -- the batch for mhpc_solve, the list for mhpc_tick_problems -- and a
 *    problem with a smaller budget sits the rest out, as it would in a handle of its own
 *    (max_DDP_iter = 0: no sweep and no line search; max_AL_iter = 0: only the final AL update,
 *    and mhpc_initialize / mhpc_reset_problems leave that problem's SRB phases at zero states, as
 *    the reference's initialization() does -- only the first forward sweep rolls them out.  If
 *    such a problem is given AL iterations between mhpc_initialize and the first mhpc_solve, that
 *    solve starts with the real rollout for it; the handle then counts as one whose next solve
 *    starts with a rollout, as after mhpc_update_problem, which is what mhpc_copy_problems
 *    compares between two handles).
 *    A tick that lists only budget-(1,1) problems issues a schedule of that length.
 *  - Giving a problem a record is the reference's `_option = o` on that controller.  The fields a
 *    solve does not rewrite (budgets, thresholds, gamma, update_relax, update_ReB,
 *    update_regularization, AL_active; smooth_active is carried and reported) take effect at that
 *    problem's next solve or tick; mhpc_rollout_costs and the policy rollouts read the current
 *    AL_active.  ReB_active and update_penalty are rewritten inside a solve
 *    (MultiPhaseDDP.cpp:178-183, 273-277): for a problem whose record changed in any field they
 *    are overwritten with the new record's values.  A problem whose record did not change keeps
 *    its whole device state bit for bit, and a call that changes no problem changes nothing.
 *    mhpc_initialize and mhpc_reset_problems restore each problem's own record.
 *  - Nothing becomes pending: the calls are allowed before and after mhpc_initialize and between
 *    any two other calls.  Device work is proportional to the number of changed problems.
 *  - A refused call changes nothing. */
int mhpc_set_options(mhpc_handle* h, const mhpc_hsddp_option* opt);   /* every problem */
int mhpc_get_options(mhpc_handle* h, mhpc_hsddp_option* opt);         /* problem 0's */
int mhpc_set_option_sets(mhpc_handle* h, int n_sets, const mhpc_hsddp_option* sets,
                         const int32_t* set_of_problem);
int mhpc_get_problem_options(mhpc_handle* h, int problem, mhpc_hsddp_option* opt);
/* Distinct option sets in use (1 for a fresh handle). */
int mhpc_num_option_sets(mhpc_handle* h, int* n);

/* Running-cost gradient lx of knots 0..N-2 ([batch][N-1][n]) and terminal-cost gradient Phix
 * ([batch][n]) of `phase` as the last partials evaluation left them: the reference's
 * rcost_*[p][k].lx and tcost_*[p].Phix that print_debugInfo writes to cost.txt
 * (MHPCLocomotion.cpp:355-377; AL terms in Phix only after forward_sweep(0), quirk B1).
 * Either pointer may be NULL. */
int mhpc_get_cost_gradients(mhpc_handle* h, int phase, double* lx, double* Phix);
/* The same for problems [first, first + count) (rows of count in place of batch); with
 * per-problem layouts the range's phase must have one shape. */
int mhpc_get_cost_gradients_problems(mhpc_handle* h, int phase, int first, int count, double* lx,
                                     double* Phix);

/* The trial rollouts of MultiPhaseDDP::forward_iteration (MultiPhaseDDP.cpp:130-151, i.e.
 * SinglePhase::forward_sweep_dynamics_only, SinglePhase.cpp:117-144, chained over phases by
 * MultiPhaseDDP::forward_sweep_dynamics_only :56-76) at n_eps arbitrary step sizes, from the
 * handle's current nominal, gains and AL/ReB state (after mhpc_solve, or right after
 * mhpc_initialize), costs only, nothing modified: J = actual cost, viol = terminal-
 * constraint violation, both [batch][n_eps].  ms (optional) = device time of the launch.
 * The C2 workload (256 concurrent rollouts of one nominal). */
#define MHPC_MAX_ROLLOUT_EPS 4096
int mhpc_rollout_costs(mhpc_handle* h, int n_eps, const double* eps, double* J, double* viol,
                       float* ms);

/* ---- policy rollouts: the batch axis over measured / perturbed start states ------------
 * A solve leaves a feedback policy on the device: per knot a nominal x, u and a gain K, run as
 * u = u_k + K_k (x - x_k) from the state the robot is actually in.  The reference spells this
 * set_initial_condition(x) followed by forward_sweep_dynamics_only(0)
 * (HSDDPSolver/source/SinglePhase.cpp:117-144; MultiPhaseDDP.cpp:56-76 chains it over phases
 * through phase_transition).  Here every problem runs n_samples start states of the caller's
 * choosing through its policy in one launch (lane = (problem, sample), the line search's own
 * model, costs and transitions, bit for bit mhpc_rollout_costs at step size 0 from that state).
 * Nothing the handle owns is modified, except x0 by mhpc_advance_x0.  All four return
 * MHPC_ERR_STATE before mhpc_initialize (or after mhpc_set_layouts until the next one) and, but
 * mhpc_get_x0, while commands or constraint parameters are pending (as mhpc_rollout_costs); a
 * pending x0 does not block them, they do not read the handle's x0.  MHPC_ERR_INVALID: a null
 * required pointer, n_samples outside 1..MHPC_MAX_POLICY_SAMPLES, n_phases out of range, a
 * non-finite entry of xs / dx, a bad problem range or a ragged phase shape.  A refused call
 * changes nothing. */
#define MHPC_MAX_POLICY_SAMPLES 4096
/* xs: [batch][n_samples][r], r = the x0 row length of mhpc_set_x0 (14 if any layout has a
 * whole-body phase, else 6; an SRB-only problem reads the first 6).  n_phases: 1..the
 * smallest phase count over the problems' layouts, or 0 = every phase of each problem.
 * J, viol: [batch][n_samples]; x_end: [batch][n_samples][r]; viol, x_end, ms may be NULL.
 * J sums the rolled phases' costs, viol = sqrt(sum h^2) over them.  x_end is the state after the
 * last rolled phase's transition: after a whole-body phase the full 14-entry state after the
 * impact, before the SRB projection (the robot's state, usable as the next x0); after an SRB
 * phase 6 entries, the rest of the row zero; after a problem's last phase its terminal state. */
int mhpc_rollout_policy(mhpc_handle* h, int n_samples, const double* xs, int n_phases,
                        double* J, double* viol, double* x_end, float* ms);
/* Trajectories of `phase` (rolled from phase 0) for problems [first, first+count), whose
 * phase must have one shape (as mhpc_get_phase_problems).  xs: [count][n_samples][r];
 * x: [count][n_samples][N][xsize], u, y: [count][n_samples][N][4] (last knot's u, y rows
 * zero; SRB y zero); any output may be NULL. */
int mhpc_rollout_policy_phase(mhpc_handle* h, int phase, int first, int count, int n_samples,
                              const double* xs, double* x, double* u, double* y);
/* Device-side closed loop: x0[b] <- x_end of one policy rollout of problem b over n_phases
 * (>= 1) phases from x0[b] + dx[b] (dx [batch][r], NULL = zero), no host copy of states.
 * Afterwards the handle is as after mhpc_set_x0 (mhpc_solve refuses until
 * mhpc_update_problem(s) / mhpc_initialize).  MHPC_ERR_INVALID if, for a problem that has a
 * whole-body phase, phase n_phases-1 is an SRB phase (its end state cannot start a
 * whole-body horizon). */
int mhpc_advance_x0(mhpc_handle* h, int n_phases, const double* dx);
int mhpc_get_x0(mhpc_handle* h, double* x0);   /* [batch][r], the device's current rows */

/* ---- device-resident control I/O: measured states in, feedback controls out ---------------
 * What a controller exchanges with the outside every tick: the measured state going in
 * (set_initial_condition, MultiPhaseDDP.h:24-25) and the control coming out, one knot of
 * forward_sweep_dynamics_only: u = u_nom + K (x - x_nom) (HSDDPSolver/source/SinglePhase.cpp:
 * 117-144).  The reference's controller is one object on one CPU and has no such call; a fleet
 * in a GPU simulator keeps its states and actions in device arrays, and these entry points read
 * and write them there, with no host copy of states, controls or gains.
 *  - Control steps.  A problem's policy is addressed by an integer control step j, not by a time.
 *    Problem b's steps cover its whole-body phases if it has any, else (an SRB-only problem) all
 *    its phases; phase p contributes N[p] - 1 steps (its last knot has no control), so step j is
 *    knot j - off_p of the phase p with off_p <= j < off_p + N[p] - 1.  mhpc_num_control_steps
 *    counts them for one problem.  The map follows the problem's current layout
 *    (mhpc_update_problem(s) shift it) and nominal trajectory.
 *  - The state size is n = 14 (whole-body steps) or 6 (SRB-only problem); a problem reads the
 *    first n entries of its row of r (r as in mhpc_set_x0).
 *  - Arithmetic: exactly the policy rollouts' control law at that knot,
 *    (u_nom[i] + 0 * du[i]) + sum_c K[i][c] (x[c] - x_nom[c]) summed in column order: both
 *    flavours give the bits mhpc_rollout_policy_phase reports for the knot when x is the state that
 *    rollout had there, in both precisions (tests/test_gpu_control.py).  Inputs are rounded to the
 *    handle's arithmetic type on the way in, outputs widened for a double buffer or rounded to
 *    nearest for a float buffer of an fp64 handle.  u is not clamped to the torque limit (the
 *    reference's rollout does not clamp).
 *  - Call order: as the policy rollouts.  MHPC_ERR_STATE before mhpc_initialize (or after
 *    mhpc_set_layouts until the next one) and while commands or constraint parameters are
 *    pending; a pending x0 does not block them.  Right after mhpc_initialize the policy is the PD
 *    warm start with zero gains (u == u_nom).  They modify nothing.
 *  - MHPC_ERR_INVALID, before anything is launched or changed: a null required pointer, a step
 *    outside 0..n-1 for its problem, dtype not MHPC_DEV_F64 / MHPC_DEV_F32, ldx < r or ldu < 4, a
 *    device pointer that hipPointerGetAttributes does not report as device memory of the handle's
 *    device.  mhpc_control also refuses a non-finite entry of x; the device flavours do not
 *    inspect values: a non-finite input gives a non-finite output and nothing worse (no index
 *    depends on a value).
 *  - Streams (device flavours): the library's work is ordered after everything queued on `stream`
 *    (the caller's hipStream_t; NULL = the null stream) at the call -- an event recorded there,
 *    which the handle's own stream waits for --, and like every other entry point the call returns
 *    only after its own work has finished: outputs are then visible to any stream.  The caller's
 *    stream itself is never synchronised with the host. */
#define MHPC_DEV_F64 0
#define MHPC_DEV_F32 1
int mhpc_num_control_steps(mhpc_handle* h, int problem, int* n);

/* host flavour: step [batch] (NULL = step 0 for every problem), x [batch][r];
 * outputs, each optional: u [batch][4], x_nom [batch][r] (zero past n), u_nom [batch][4],
 * K [batch][4][r] row-major (zero past column n).  x may be NULL only if u is NULL. */
int mhpc_control(mhpc_handle* h, const int32_t* step, const double* x, double* u,
                 double* x_nom, double* u_nom, double* K);

/* device flavour: step stays a host array; x, u are device arrays of dtype with row strides
 * ldx >= r, ldu >= 4 in elements (slices of a simulator's state / action tensors);
 * x_nom, u_nom, K optional, dense, same dtype.  stream: the caller's hipStream_t (NULL = the
 * null stream). */
int mhpc_control_device(mhpc_handle* h, const int32_t* step, const void* x, int64_t ldx,
                        void* u, int64_t ldu, void* x_nom, void* u_nom, void* K, int dtype,
                        void* stream);

/* mhpc_set_x0 from a device array: rows of r at x0 + b*ld, dtype as above.  Afterwards the handle
 * is in every respect as after mhpc_set_x0 of the same values (the device rows bit for bit, an
 * SRB-only problem's row tail zero, x0 pending for the next mhpc_initialize /
 * mhpc_update_problem(s)).  MHPC_ERR_INVALID for a null or non-device x0, ld < r or a bad dtype. */
int mhpc_set_x0_device(mhpc_handle* h, const void* x0, int64_t ld, int dtype, void* stream);

/* ---- device-resident plan export: policy windows and results into device arrays ------------
 * What a solve produces, for callers that keep it on the device: the next W control steps of
 * each listed problem's policy (a simulator that sub-steps between re-plans applies
 * u = u_nom + K (x - x_nom) itself) and the scalars of its last solve (a learner's dataset).
 * There is no host flavour: mhpc_get_phase(_problems) and mhpc_get_scalars are the host getters,
 * and every value here is exactly what they report.
 *  - Addressing.  Steps are the control steps of mhpc_control (above): the whole-body phases of
 *    a problem that has any, all phases of an SRB-only problem, N[p] - 1 steps a phase, by the
 *    problem's current layout and nominal trajectory.  Row i of every output belongs to
 *    problems[i]: a host list of n entries, each in range and none twice; NULL: n == batch, in
 *    order.  first_step: a host array of n entries (NULL: 0 for every problem),
 *    0 <= first_step[i] < mhpc_num_control_steps(problems[i]).  1 <= window <= MHPC_MAX_KNOTS.
 *    Window row w of problem i is step first_step[i] + w; a window runs across phase boundaries
 *    exactly as consecutive steps do (a phase's last knot, which has no control, is no step).
 *    valid[i] = min(window, steps of the problem - first_step[i]).
 *  - Values.  r is the handle's x0 row length (14 or 6); the problem's state size is n.  x_nom,
 *    u_nom, y: the knot's record of the nominal trajectory; K: the knot's 4 x n gain, row-major in
 *    rows of r; du: the feed-forward row; Vx: the value gradient; mode: the mode 1..4 of the
 *    step's phase.  Entries past n (columns of x_nom, Vx and of K's rows, for an SRB-only problem
 *    in rows of 14) are +0, and so is every row past valid (mode 0).  Nothing is written outside
 *    the [window][c] block of a listed problem: a caller's padding between blocks (ld_* larger
 *    than dense) keeps its bytes.  No arithmetic but the element-type conversion of the control
 *    I/O: widened exactly for a double array, rounded to nearest for a float array of an fp64
 *    handle or of the results' scalars (which are double in both precisions).
 *  - Results: J, dV_exp, viol, V_phase, dV_phase as mhpc_get_scalars reports them (V_phase,
 *    dV_phase in rows of P = mhpc_max_phases, zero past a problem's own phases), status as
 *    mhpc_solve reports it.
 *  - Call order, refusals and streams as mhpc_control_device: MHPC_ERR_STATE before
 *    mhpc_initialize (or after mhpc_set_layouts until the next one) and while commands or
 *    parameters are pending, a pending x0 does not block; right after mhpc_initialize the policy is
 *    the PD warm start (K = 0, Vx = 0).  MHPC_ERR_INVALID, before anything is launched: a null
 *    out, no array wanted, a bad list, first step, window or dtype, an ld_* that is neither 0 nor
 *    at least the dense block, a pointer that is not device memory of the handle's device.  A
 *    refused call changes nothing, and no call modifies anything the handle owns.  The work is
 *    ordered behind everything queued on `stream` at the call and has finished when the call
 *    returns.  ms (optional): the device time of the launch. */
typedef struct {
  /* each array optional (NULL = not wanted); ld_* = elements between two listed problems'
     blocks, 0 = dense, otherwise >= the dense block size */
  void* x_nom;   int64_t ld_x_nom;  /* [n][W][r]                                            */
  void* u_nom;   int64_t ld_u_nom;  /* [n][W][4]                                            */
  void* K;       int64_t ld_K;      /* [n][W][4][r] row-major                               */
  void* du;      int64_t ld_du;     /* [n][W][4]                                            */
  void* Vx;      int64_t ld_Vx;     /* [n][W][r]                                            */
  void* y;       int64_t ld_y;      /* [n][W][4]                                            */
  int32_t* mode; int64_t ld_mode;   /* [n][W] mode 1..4 of the step's phase; 0 past `valid` */
  int32_t* valid;                   /* [n] steps of the window that exist                   */
} mhpc_plan_out;

int mhpc_export_plan_device(mhpc_handle* h, int n, const int32_t* problems,
                            const int32_t* first_step, int window, const mhpc_plan_out* out,
                            int dtype, void* stream, float* ms);

typedef struct {
  void *J, *dV_exp, *viol;     /* [n]        */
  void *V_phase, *dV_phase;    /* [n][P], P = mhpc_max_phases, zero past a problem's own phases */
  int32_t* status;             /* [n] mhpc_solve_status of the problem's last solve */
} mhpc_results_out;

int mhpc_export_results_device(mhpc_handle* h, int n, const int32_t* problems,
                               const mhpc_results_out* out, int dtype, void* stream);

/* ---- device-resident plan import: warm-start listed problems from device arrays -------------
 * The other direction of mhpc_export_plan_device: "start problem b from these controls".  The
 * nominal controls of the listed problems at a window of steps are overwritten, optionally the
 * gains and the nominal states they refer to as well, and the problems are marked so that the
 * first forward_sweep(0) of their next mhpc_solve / mhpc_tick_problems is the real rollout of
 * u = u_nom + K (x - x_nom) from x0, exactly as after mhpc_update_problem(s).  Nothing else changes.
 *  - Steps.  scope chooses the step map.  MHPC_STEPS_CONTROL: the control steps of mhpc_control
 *    and mhpc_export_plan_device -- the whole-body phases of a problem that has any (the scope of
 *    the reference's warmstart(); the SRB phases keep what they hold, zero controls after
 *    mhpc_initialize), all phases of an SRB-only problem; an exported window can be imported as it
 *    is.  MHPC_STEPS_ALL: every phase of the problem in order.  Either way phase p contributes
 *    N[p] - 1 steps (its last knot has no control), by the problem's current layout.
 *    mhpc_num_plan_steps counts a problem's steps under a scope.
 *  - Addressing as the export's: row i belongs to problems[i] (a host list of n entries, each in
 *    range and none twice; NULL: n == batch, in order); first_step a host array of n entries
 *    (NULL: 0), 0 <= first_step[i] < mhpc_num_plan_steps(problems[i], scope); 1 <= window <=
 *    MHPC_MAX_KNOTS; window row w is step first_step[i] + w; rows past the problem's valid =
 *    min(window, steps - first_step[i]) are ignored.  ld_* = elements between two listed
 *    problems' blocks, 0 = dense.
 *  - Values.  r is the handle's x0 row length (14 or 6); a step's state size n is its phase's: 14
 *    in a whole-body phase, 6 in an SRB phase.  u_nom [n][W][4] (required) goes into entries
 *    n..n+4 of the knot's record in the problem's current nominal trajectory; x_nom [n][W][r] into
 *    entries 0..n; K [n][W][4][r], row-major, into the knot's dense 4 n gain words.  Columns past n
 *    (of x_nom and of K's rows) are not read.  K is optional and x_nom required exactly when K is
 *    given.  Without K the written knots' 56 gain words become +0 -- the guess is open-loop -- and
 *    their x_nom entries stay.  Never written: y, du, Vx, any other trajectory, the partials, the
 *    problem's state and scalars, any knot outside the window, any unlisted problem.  (The rollout
 *    at eps = 0 multiplies du by zero, and the next backward sweep rewrites du and Vx before
 *    anything reads them.)  Element types: widened exactly, rounded to nearest into an fp32
 *    handle.  The device flavour does not inspect values: a non-finite guess ends as
 *    MHPC_SOLVE_NONFINITE like any problem that blows up.  The host flavour (dense double arrays,
 *    staged into the same kernel) refuses non-finite entries among those it would read.
 *  - Call order.  A problem that has been given a guess stops being fresh (mhpc_reset_problems):
 *    its next first sweep is the rollout.  On a handle that is initialised and not yet solved with
 *    no rollout due, the next mhpc_solve starts with the rollout for the guessed problems and with
 *    the cost evaluation for all others, which therefore come out bit for bit as without the
 *    import.  A problem whose option record has max_AL_iter = 0 never rolls anything out, in the
 *    reference either: its guess stays as written.  A later mhpc_reset_problems of the same
 *    problem wins; a second import overlays the first.  Snapshots carry the marks as before.
 *  - Refusals and streams as mhpc_export_plan_device: MHPC_ERR_STATE before mhpc_initialize and
 *    while commands or parameters are pending, a pending x0 does not block.  MHPC_ERR_INVALID,
 *    before anything is written: a null `in` or u_nom, K without x_nom (or x_nom without K), a bad
 *    list, first step, window, scope or dtype, an ld_* that is neither 0 nor at least the dense
 *    block, a pointer that is not device memory of the handle's device.  A refused call changes
 *    nothing.  The work is ordered behind everything queued on `stream` at the call and has
 *    finished when the call returns.  ms (optional): the device time of the launch. */
#define MHPC_STEPS_CONTROL 0
#define MHPC_STEPS_ALL 1
typedef struct {
  const void* u_nom; int64_t ld_u_nom;  /* [n][W][4]     required                      */
  const void* K;     int64_t ld_K;      /* [n][W][4][r]  optional, row-major           */
  const void* x_nom; int64_t ld_x_nom;  /* [n][W][r]     given exactly when K is given */
} mhpc_plan_in;

int mhpc_num_plan_steps(mhpc_handle* h, int problem, int scope, int* n);
int mhpc_import_plan_device(mhpc_handle* h, int n, const int32_t* problems,
                            const int32_t* first_step, int window, int scope,
                            const mhpc_plan_in* in, int dtype, void* stream, float* ms);
int mhpc_import_plan(mhpc_handle* h, int n, const int32_t* problems, const int32_t* first_step,
                     int window, int scope, const double* u_nom, const double* K,
                     const double* x_nom);

/* Per-kernel device timing (HIP events around every launch on the handle's stream) and the
 * algorithmic HBM bytes each kernel must move (model in DESIGN.md §Roofline), accumulated
 * over all solves since the last reset.  Kernel ids: 0 init, 1 forward_sweep(0) cost,
 * 2 line search (rollouts + costs + selection), 3 partials, 4 backward_sweep (whole, or its
 * WB half when split), 5 al_update, 6 the SRB half of a split backward sweep. */
#define MHPC_NUM_KERNELS 7
const char* mhpc_kernel_name(int k);
int mhpc_set_profiling(mhpc_handle* h, int on);
int mhpc_get_kernel_stats(mhpc_handle* h, double* ms, int64_t* launches, double* alg_bytes);
int mhpc_reset_kernel_stats(mhpc_handle* h);
/* Algorithmic FP64 flops per kernel accumulated like mhpc_get_kernel_stats' bytes: the
 * backward sweep in the reference's dense formulation; 0 for the others. */
int mhpc_get_kernel_flops(mhpc_handle* h, double* flops);
void mhpc_destroy(mhpc_handle* h);

/* Kernel variants.  The launch shape of the backward sweep and of the line search is chosen
 * from the batch size and the device's compute-unit count; every variant
 * computes the same per-problem arithmetic, bit for bit (tests/test_gpu_variants.py).  This
 * call pins one variant for the handle's later solves -- for parity tests of every variant
 * at any batch size, and for tuning.  variant 0 restores the automatic choice.
 * MHPC_ERR_INVALID if the variant does not apply (the staged line-search variants need at
 * least 10 line-search candidates, the pair variant at most 32). */
#define MHPC_VARIANT_BWS 0            /* which: backward sweep */
#define MHPC_VARIANT_BWS_ROWS4 1      /*   four problems per wave (one per 16-lane row) */
#define MHPC_VARIANT_BWS_ROWS2 2      /*   two problems per wave (rows 0, 1) */
#define MHPC_VARIANT_BWS_ROWS1 3      /*   one problem per wave (row 0) */
#define MHPC_VARIANT_BWS_PAIRS2 4     /*   two problems per wave, two rows each in the
                                         whole-body phases (default up to 2048 problems) */
#define MHPC_VARIANT_RO 1             /* which: line-search rollouts */
#define MHPC_VARIANT_RO_PAIR 1        /*   two-wave pipeline, a lane pair per candidate */
#define MHPC_VARIANT_RO_PIPE_STAGED 2 /*   two-wave pipeline, LDS-staged operands */
#define MHPC_VARIANT_RO_PIPE 3        /*   two-wave pipeline, operands from HBM */
#define MHPC_VARIANT_RO_FUSED_STAGED 4 /*  one wave, LDS-staged operands */
#define MHPC_VARIANT_RO_FUSED 5       /*   one wave, operands from HBM */
#define MHPC_VARIANT_OVERLAP 2        /* which: partials beside the SRB half of the sweep */
#define MHPC_VARIANT_OVERLAP_ON 1     /*   two launches + second stream (default when both
                                         WB and SRB phases are present) */
#define MHPC_VARIANT_OVERLAP_OFF 2    /*   one sweep launch after the partials */
#define MHPC_VARIANT_SUBBATCH 3       /* which: sub-batches run concurrently; variant = their
                                         count 1..MHPC_MAX_SUBBATCH (contiguous blocks of the
                                         batch, one stream pair each, staggered by one launch
                                         so that one block's line search shares the chip with
                                         another block's sweep); 0 = automatic */
#define MHPC_MAX_SUBBATCH 4
#define MHPC_VARIANT_RO_STORE 4       /* which: line-search trials that store their knot
                                         records: the first `variant` (1..32) and the last;
                                         an accepted trial without records is rolled out again
                                         into its slot (same arithmetic, bit for bit);
                                         0 = the default (4) */
#define MHPC_VARIANT_SWEEP_BITS 5     /* which: arithmetic of the backward sweep: 64 (default,
                                         also in an fp32 handle, whose sweep reads float records
                                         and writes float gains but sums, factors and carries the
                                         value function in double) or, fp32 handles only, 32
                                         (the sweep in float, its 4x4 control block in double:
                                         no faster -- within 1 % of the double sweep -- and 10-70x
                                         larger typical error vs the fp64 oracle, DESIGN.md §3,
                                         §5); 0 = default */
#define MHPC_VARIANT_SNAP_ROUND 6     /* which: problems a round of mhpc_snapshot_problems /
                                         mhpc_restore_problems (variant = R >= 1; 0 = as many as
                                         fit the staging cap); any R gives the same blob and the
                                         same restore, byte for byte */
int mhpc_set_kernel_variant(mhpc_handle* h, int which, int variant);

/* ---- batched model evaluation on the device (kernel-level parity hooks) -----------
 * Replace the CasADi C ABI of SURVEY.md table 2b for whole batches of points.  All
 * arrays are host, row-major, n points.  Dense outputs: Ac/Px [n][14][14], Bc [n][14][4],
 * C [n][4][14], D [n][4][4]; SRB Ac [n][6][6], Bc [n][6][4]. */
int mhpc_eval_wb_dynamics(int device, int n, int mode, const double* x, const double* u,
                          double* xdot, double* y);
/* The line search's lane-pair evaluation of the same dynamics (mhpc_model_pair.h: even lane
 * front leg, odd lane back leg): xdot [n][2][14], y [n][2][4] hold what each lane of the pair
 * computed; both must equal mhpc_eval_wb_dynamics bit for bit. */
int mhpc_eval_wb_dynamics_pair(int device, int n, int mode, const double* x, const double* u,
                               double* xdot, double* y);
/* Touchdown constraint WB_FL1 (foot 0: front, used at the end of mode 2) / WB_FL2 (foot 1:
 * back, mode 4) and the foot Jacobian Jacob_F / Jacob_B, as the kernels evaluate them:
 * h [n][2] (the derivative routine's value, then the value-only routine's), hx [n][14],
 * hxx [n][14][14], J and Jd [n][2][7] (row-major). */
int mhpc_eval_wb_touchdown(int device, int n, int foot, const double* x, double* h, double* hx,
                           double* hxx, double* J, double* Jd);
/* The same two models in the fp32 instantiation (config C5): pair = 0 single lane (xdot
 * [n][14], y [n][4]), pair = 1 lane pair (xdot [n][2][14], y [n][2][4]); double host arrays,
 * inputs rounded to float. */
int mhpc_eval_wb_dynamics_f32(int device, int n, int mode, int pair, const double* x,
                              const double* u, double* xdot, double* y);
int mhpc_eval_wb_partials(int device, int n, int mode, const double* x, const double* u,
                          double* Ac, double* Bc, double* C, double* D);
int mhpc_eval_wb_impact(int device, int n, int foot, const double* x, double* xplus,
                        double* Px);
int mhpc_eval_srb(int device, int n, const double* x, const double* u, const double* foothold,
                  const double* contact, double* xdot, double* Ac, double* Bc);
/* The fp32 instantiation's build of the same kernels: the signatures and output shapes of the
 * hooks above, double host arrays, inputs rounded to float and float results widened. */
int mhpc_eval_wb_partials_f32(int device, int n, int mode, const double* x, const double* u,
                              double* Ac, double* Bc, double* C, double* D);
int mhpc_eval_wb_impact_f32(int device, int n, int foot, const double* x, double* xplus,
                            double* Px);
int mhpc_eval_wb_touchdown_f32(int device, int n, int foot, const double* x, double* h,
                               double* hx, double* hxx, double* J, double* Jd);
int mhpc_eval_srb_f32(int device, int n, const double* x, const double* u,
                      const double* foothold, const double* contact, double* xdot, double* Ac,
                      double* Bc);

/* ---- hand-written elementary functions on the device (accuracy hooks) ---------------
 * Each function evaluated at n points exactly as the solve kernels call it.  Lane i of a
 * 64-lane block takes point i (of the SINCOS_N functions: group i of 5 / 3 consecutive angles,
 * n a multiple of the group), so the caller decides which arguments share a wavefront.
 * Host arrays are double, rounded to the library's type on the way in and widened on the way
 * out; b is read by REDUCED_BARRIER and DIV_CONST only (else it may be null).
 * out: [n][2] (sin, cos), [n][3] (B, Bz, Bzz) or [n]. */
#define MHPC_PRIM_SINCOS 0          /* sin_cos(a) */
#define MHPC_PRIM_SINCOS_N5 1       /* sin_cos_n<5> (whole-body geometry) */
#define MHPC_PRIM_SINCOS_N3 2       /* sin_cos_n<3> (lane-pair model) */
#define MHPC_PRIM_SINCOS_N5_VK 3    /* the same two with the knot loops' register copy of */
#define MHPC_PRIM_SINCOS_N3_VK 4    /* the reduction constants */
#define MHPC_PRIM_PIVOT_RCP 5       /* pivot_rcp(a) (model pivots) */
#define MHPC_PRIM_SWEEP_RECIP 6     /* the backward sweep's recip(a) in the sweep's type: double
                                       in both libraries (a and out are not rounded) */
#define MHPC_PRIM_SWEEP_RECIP_F32 7 /* mhpc_eval_primitive_f32 only: recip(float) of the float
                                       sweep (MHPC_VARIANT_SWEEP_BITS 32) */
#define MHPC_PRIM_LOG_POS 8         /* log_pos(a) */
#define MHPC_PRIM_REDUCED_BARRIER 9 /* reduced_barrier(g = a, delta = b) */
#define MHPC_PRIM_DIV_CONST 10      /* div_const(a, c, RN(1 / c)): c the SRB mass (b = 0) or the
                                       SRB inertia (b != 0) */
int mhpc_eval_primitive(int device, int fn, int n, const double* a, const double* b, double* out);
int mhpc_eval_primitive_f32(int device, int fn, int n, const double* a, const double* b,
                            double* out);

#ifdef __cplusplus
}
#endif
#endif /* MHPC_CAPI_H */
