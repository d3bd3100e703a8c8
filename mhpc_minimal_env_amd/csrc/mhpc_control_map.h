// The control-step map of mhpc_control / mhpc_control_device: which knot of a problem's packed
// arrays holds the policy of control step j, and where that knot's nominal record, gain block
// and feed-forward row lie.
//
// A problem's policy is addressed by an integer control step, never by a time (a time divided by
// dt at a knot boundary rounds either way).  The steps cover the problem's whole-body phases when
// it has any -- an SRB phase's control is a ground-reaction force, nothing to apply to the robot --
// and all its phases when it is SRB-only.  Phase p contributes N[p] - 1 steps (its last knot has
// no control), so step j is knot k = j - off_p of the phase p with off_p <= j < off_p + N[p] - 1,
// off_p = sum over q < p of (N[q] - 1).  The knot's index in the packed arrays is ko[p] + k with
// the layout's own ko (the layout of the problem as mhpc_update_problem(s) left it), and its
// nominal record lies in the trajectory slot the problem's state names (nom_slot).
//
// The kernel (mhpc_control.hip), the host validation (mhpc_runtime.cpp) and the host check
// (tests/native/control_map_hostcheck.cpp) run the same code; everything here is plain integer
// arithmetic on the layout, no index comes from array contents.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MHPC_CTRL_HD __host__ __device__
#else
#define MHPC_CTRL_HD
#endif

namespace mhpc_ctrl {

// record widths of mhpc_solver.h (mhpc_control.hip asserts that they agree)
constexpr int KS = 24, KW = 56, UW = 4, XW = 14;

// Phases whose knots are control steps, and the state size of those phases.
MHPC_CTRL_HD inline int n_phases(int P, int n_wb) { return n_wb > 0 ? n_wb : P; }
MHPC_CTRL_HD inline int state_size(int n_wb) { return n_wb > 0 ? 14 : 6; }

MHPC_CTRL_HD inline int n_steps(int P, int n_wb, const int* N) {
  int n = 0;
  for (int p = 0; p < n_phases(P, n_wb); ++p) n += N[p] - 1;
  return n;
}

struct Knot {
  int phase, k;  // the phase and the knot within it, k < N[phase] - 1
  int kk;        // the knot's index in the problem's packed arrays: ko[phase] + k
};
// Control step j of a layout; false (and *o untouched) for a step outside [0, n_steps).  Every
// phase is visited, so lanes with different steps run the same instructions.
MHPC_CTRL_HD inline bool knot_of(int P, int n_wb, const int* N, const int* ko, int j, Knot* o) {
  bool found = false;
  int off = 0;
  for (int p = 0; p < n_phases(P, n_wb); ++p) {
    const int n = N[p] - 1;
    if (j >= off && j < off + n) {
      o->phase = p;
      o->k = j - off;
      o->kk = ko[p] + (j - off);
      found = true;
    }
    off += n;
  }
  return found;
}

// Element offsets of knot kk of problem b: its record in trajectory slot `slot` of traj
// [B][nslot][NK][KS] (x first, then u), its gain block in K [B][NK][56] (4 rows of the state
// size, dense) and its feed-forward row in du [B][NK][4].
MHPC_CTRL_HD inline size_t nom_off(int NK, int nslot, int b, int slot, int kk) {
  return (((size_t)b * nslot + slot) * NK + kk) * KS;
}
MHPC_CTRL_HD inline size_t gain_off(int NK, int b, int kk) { return ((size_t)b * NK + kk) * KW; }
MHPC_CTRL_HD inline size_t du_off(int NK, int b, int kk) { return ((size_t)b * NK + kk) * UW; }

}  // namespace mhpc_ctrl
