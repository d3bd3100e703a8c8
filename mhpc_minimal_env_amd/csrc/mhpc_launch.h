// What the kernel translation units (mhpc_kernels.hip, mhpc_bws.hip, ...) export to the host
// runtime: the launchers, the launch-shape queries, and the record widths the host unpacks.
// Included by both kernel files and by mhpc_runtime.cpp, so a prototype that no longer matches
// its definition fails to compile instead of failing to link.
#pragma once
#include <hip/hip_runtime.h>

#include "mhpc_solver.h"

namespace MHPC_NS {

// Blocks of a launch over the groups with `per` problems a block (block_group)
static inline unsigned grid_of(const SolveParams& sp, int per) {
  long n = 0;
  for (int g = 0; g < sp.ngrp; ++g) n += (sp.go[g + 1] - sp.go[g] + per - 1) / per;
  return (unsigned)n;
}
// ... and with items[g] (or n_items) work items per problem, nt a block (block_group_items)
static inline unsigned grid_items(const SolveParams& sp, const int* items, int n_items, int nt) {
  long n = 0;
  for (int g = 0; g < sp.ngrp; ++g)
    n += ((long)(sp.go[g + 1] - sp.go[g]) * (items ? items[g] : n_items) + nt - 1) / nt;
  return (unsigned)n;
}

// ---- mhpc_kernels.hip -----------------------------------------------------------------------
hipError_t launch_cost(const SolveParams& sp, const DevBufs& d, int al_iter, hipStream_t s);
hipError_t launch_rollout(const SolveParams& sp, const DevBufs& d, int al_iter, int ddp_iter,
                          int full, hipStream_t s);
// (al_iter, ddp_iter: the op of the solve schedule a launch belongs to -- every kernel of the
// schedule leaves out the problems whose own iteration caps exclude that op, in_op, mhpc_device.h)
hipError_t launch_partials(const SolveParams& sp, const DevBufs& d, int al_iter, int ddp_iter,
                           hipStream_t s, hipStream_t s3, hipEvent_t fork, hipEvent_t join);
hipError_t launch_al_end(const SolveParams& sp, const DevBufs& d, int al, int last, hipStream_t s);
hipError_t launch_reduce_counters(const SolveParams& sp, const DevBufs& d,
                                  unsigned long long* out, hipStream_t s);
int launch_problems(const SolveParams& sp);  // problems of a launch (a sub-batch's share)
int ro_store_default();
int ro_store_auto(const SolveParams& sp);

// the serial rollouts beside the schedule and the debug gradient: not part of a solve, kept in
// mhpc_kernels.hip because k_policy_rollout's code changes without k_partials_impact beside it
// (profiles/kernels_split_ab.md)
hipError_t launch_cost_grad(const SolveParams& sp, const DevBufs& d, int g, int p, int N, int b0,
                            int nb, real* lx, real* phix, hipStream_t s);
hipError_t launch_eps_rollout(const SolveParams& sp, const DevBufs& d, int n_eps,
                              const real* eps, real* J, real* viol, hipStream_t s);
constexpr int PREC_W = 22;  // k_policy_rollout's knot record: x 14, u 4, y 4
hipError_t launch_policy_rollout(const SolveParams& sp, const DevBufs& d, int n_s, int b0, int nb,
                                 const real* xs, const double* dx, int n_phases, int rec_p,
                                 real* J, real* viol, real* xe, real* rec, hipStream_t s);

// ---- mhpc_init.hip --------------------------------------------------------------------------
hipError_t launch_init(const SolveParams& sp, const DevBufs& d, hipStream_t s);
hipError_t launch_init_params(const SolveParams& sp, const DevBufs& d, int warm, hipStream_t s);
hipError_t launch_reset(const SolveParams& sp, const DevBufs& d, hipStream_t s);
hipError_t launch_reset_arrays(const SolveParams& sp, const DevBufs& d, hipStream_t s);
// list-driven device code of mhpc_reset_problems: x0 rows [n][14] to the listed problems, and
// their memory_reset (K / du / G, last-knot tails, store rows when store != nullptr)
hipError_t launch_scatter_x0(const DevBufs& d, int n, const int* list, const real* rows,
                             hipStream_t s);
hipError_t launch_reset_list(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                             real* store, int nbk, int spmax, hipStream_t s);

// ---- mhpc_store.hip -------------------------------------------------------------------------
// Phase-buffer store of the receding-horizon loop, [B][spmax][nbk][kStoreRec]: buffers of
// N_TIMESTEPS_MAX (MHPCLocomotion.h) knots at least; record = x,u,y + K + du + G
constexpr int kPhaseBufKnots = 110;
constexpr int kStoreRec = KS + 56 + 4 + 14;
hipError_t launch_store(const SolveParams& sp, const DevBufs& d, real* store, int nbk, int spmax,
                        int save, hipStream_t s);
hipError_t launch_export(const SolveParams& sp, const DevBufs& d, hipStream_t s);
hipError_t launch_export_ref(const SolveParams& sp, const DevBufs& d, int b0, int nb, hipStream_t s);

// ---- mhpc_eval.hip --------------------------------------------------------------------------
// model evaluation hooks (n points each)
hipError_t launch_eval_wb_dyn(int n, int mode, const real* x, const real* u, real* xd,
                              real* y, hipStream_t s);
hipError_t launch_eval_wb_dyn_pair(int n, int mode, const real* x, const real* u, real* xd,
                                   real* y, hipStream_t s);
hipError_t launch_eval_wb_aux(int n, int foot, const real* x, real* h, real* hx, real* hxx,
                              real* J, real* Jd, hipStream_t s);
hipError_t launch_eval_wb_par(int n, int mode, const real* x, const real* u, real* Ac,
                              real* Bc, real* C, real* D, hipStream_t s);
hipError_t launch_eval_wb_impact(int n, int foot, const real* x, real* xp, real* Px,
                                 hipStream_t s);
hipError_t launch_eval_srb(int n, const real* x, const real* u, const real* p,
                           const real* c, real* xd, real* Ac, real* Bc, hipStream_t s);

// primitive evaluation hook (MHPC_PRIM_*): n points, out [n][2 | 3 | 1]; eval_prim_group = the
// angles one lane takes (5 / 3 of the sin_cos_n functions, else 1), which n is a multiple of
int eval_prim_group(int fn);
hipError_t launch_eval_prim(int fn, int n, const real* a, const real* b, real* out,
                            hipStream_t s);

// ---- mhpc_copy.hip --------------------------------------------------------------------------
// One side of mhpc_copy_problems: a handle's arrays with their knot stride and the shape of its
// phase-buffer store (store == nullptr: the handle has none).  pairs [n][2] on the device: source
// problem, destination problem; blocks [nblk]: the (run, chunk) table of one pair, which
// copy_block_table writes (out may be null) and counts; the re-stride map is mhpc_copy_map.h.
struct CopySide {
  DevBufs d;
  real* store;
  int NK, nslot, nbk, spmax;
};
int copy_block_table(const CopySide& src, const CopySide& dst, int* out);
hipError_t launch_copy_problems(const CopySide& src, const CopySide& dst, int n, const int* pairs,
                                int nblk, const int* blocks, hipStream_t s);

// ---- mhpc_snapshot.hip ----------------------------------------------------------------------
// The staging side of one round of mhpc_snapshot_problems / mhpc_restore_problems: R problems of
// knot stride NK, nslot slots and a store of spmax buffers of nbk knots (spmax = 0: none) laid out
// in one device buffer of snap_stage_bytes (mhpc_snapshot_map.h) -- a CopySide, so pack and unpack
// are launch_copy_problems into and out of it.  snap_move queues the copies of `count` consecutive
// entries between a blob's payload (n entries) from `entry` on and the staging records from `slot`
// on, one per array.
CopySide snap_side(void* staging, int R, int NK, int nslot, int nbk, int spmax);
size_t snap_stage_bytes(int R, int NK, int nslot, int nbk, int spmax);
hipError_t snap_move(void* staging, int R, int NK, int nslot, int nbk, int spmax, char* payload,
                     int n, int entry, int slot, int count, bool to_host, hipStream_t s);

// ---- mhpc_tick.hip --------------------------------------------------------------------------
// list-driven device code of mhpc_tick_problems: the phase-buffer save (save = 1: the nominal slot
// of each listed problem to its store rows) / load (store rows to slot 0, K, du, G; a phase's last
// knot to every slot) by each problem's own layout d.grp[d.lid[b]], and the listed problems'
// status words to status [n] on the device, in list order
hipError_t launch_store_list(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                             real* store, int nbk, int spmax, int save, hipStream_t s);
hipError_t launch_status_list(const DevBufs& d, int n, const int* list, int32_t* status,
                              hipStream_t s);

// ---- mhpc_options.hip -----------------------------------------------------------------------
// list-driven device code of mhpc_set_option_sets / mhpc_copy_problems: ent [n][2] on the device,
// (problem, option record); each listed problem's oid entry and, with state != 0, the option
// fields a solve rewrites (ProbState::opt_reb / opt_pen) from that record of the table
// (oid: the handle's writable index, the array d.oid reads)
hipError_t launch_set_options(const DevBufs& d, int* oid, int n, const int* ent, int state,
                              hipStream_t s);

// ---- mhpc_control.hip -----------------------------------------------------------------------
// Control I/O through device arrays of the caller's element type (dtype MHPC_DEV_F64 / _F32).
// launch_control: u = u_nom + K (x - x_nom) at control step step[b] of every problem (step on the
// device, null: step 0; the step map is mhpc_step_map.h under STEPS_CONTROL and the host has
// checked every step against it).  x rows at a stride of ldx, u rows at ldu, in elements; x_nom
// [B][r], u_nom [B][4], K [B][4][r] dense; every output may be null, x only when u is.
hipError_t launch_control(const SolveParams& sp, const DevBufs& d, const int* step, const void* x,
                          long ldx, void* u, long ldu, void* x_nom, void* u_nom, void* K, int r,
                          int dtype, hipStream_t s);
// launch_x0_in: the handle's x0 rows of 14 from rows at x0 + b * ld (mhpc_set_x0's padding)
hipError_t launch_x0_in(const SolveParams& sp, const DevBufs& d, const void* x0, long ld, int dtype,
                        hipStream_t s);

// ---- mhpc_plan_export.hip -------------------------------------------------------------------
// launch_plan_export: `window` control steps from first[i] (device, null: 0) of listed problem
// list[i] (device, null: problem i) into block i of each wanted array, by the map of
// mhpc_step_map.h under STEPS_CONTROL, whose kinds index arrays [NOUT] (null: not wanted; all of
// dtype but mode, int32) and ld [NOUT] (elements between two blocks, >= the dense block); valid
// [n] may be null.  The host has checked the list and every first step against the same map.
hipError_t launch_plan_export(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                              const int* first, int window, int r, void* const* arrays,
                              const long* ld, int32_t* valid, int dtype, hipStream_t s);
// launch_results_export: arrays [5] = J, dV_exp, viol [n], V_phase, dV_phase [n][P] of dtype
// (each may be null) and status [n] (may be null) of the listed problems, in list order
hipError_t launch_results_export(const DevBufs& d, int n, const int* list, int P,
                                 void* const* arrays, int32_t* status, int dtype, hipStream_t s);

// ---- mhpc_plan_import.hip -------------------------------------------------------------------
// launch_plan_import: `window` steps from first[i] (device, null: 0) of listed problem list[i]
// (device, null: problem i) out of block i of each given array, by the map of mhpc_step_map.h
// under `scope`, whose kinds index arrays [NIN] = x_nom, u_nom, K of dtype (u_nom given; x_nom and
// K both or neither: without them the window knots' gain words become +0) and ld [NIN] (elements
// between two blocks, >= the dense block).  The host has checked the list and every first step
// against the same map.
hipError_t launch_plan_import(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                              const int* first, int window, int scope, int r,
                              const void* const* arrays, const long* ld, int dtype,
                              hipStream_t s);

// ---- mhpc_bws.hip ---------------------------------------------------------------------------
hipError_t launch_bws(const SolveParams& sp, const DevBufs& d, int al_iter, int ddp_iter, int part,
                      hipStream_t s);
bool bws_split(const SolveParams& sp);
// the sweep's pivot reciprocal in the sweep's arithmetic type (double in both libraries)
hipError_t launch_eval_recip(int n, const double* a, double* out, hipStream_t s);
#ifdef MHPC_FP32
namespace fsweep {  // the float-arithmetic sweep (mhpc_bws.hip built with MHPC_BWS_F64=0)
hipError_t launch_bws(const SolveParams& sp, const DevBufs& d, int al_iter, int ddp_iter, int part,
                      hipStream_t s);
hipError_t launch_eval_recip(int n, const float* a, float* out, hipStream_t s);
}
#endif

}  // namespace MHPC_NS
