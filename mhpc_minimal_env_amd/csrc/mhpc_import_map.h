// The window map of mhpc_import_plan_device: which element of a problem's packed arrays an element
// of a caller's [W][c] block goes to.
//
// The inverse direction of mhpc_plan_map.h, over one of two step maps (`scope`):
//   STEPS_CONTROL  the control steps of mhpc_control_map.h: the whole-body phases of a problem that
//                  has any, all phases of an SRB-only problem.  Every step has the problem's one
//                  state size (14 or 6), so a window that mhpc_export_plan_device wrote goes back
//                  element for element.
//   STEPS_ALL      every phase of the problem in order, N[p] - 1 steps a phase (a phase's last
//                  knot has no control and is never a step).  The state size is the phase's: 14 in
//                  a whole-body phase, 6 in an SRB phase.
// A window is W consecutive steps from a first step on; its `valid` rows exist, the rows past them
// are not read.  In rows of the handle's x0 row length r the columns past the step's state size n
// are not read either.  Four kinds share the map:
//   x_nom [W][r]      -> traj record of the knot, entries 0..n          (nominal slot)
//   u_nom [W][4]      -> traj record, entries n..n+4
//   K     [W][4][r]   -> the 4 n dense words of the knot's 56, row i at i n
//   zero gains [W][56] (no input array) -> all 56 gain words of the knot: an import without K
// Nothing else of a record is ever a destination: y (entries n+4..n+8), the record's tail, du, G.
//
// The kernel (mhpc_plan_import.hip), the runtime's validation (mhpc_runtime.cpp) and the host check
// (tests/native/import_map_hostcheck.cpp) run the same code; everything here is plain integer
// arithmetic on the layout, no index comes from array contents.
#pragma once
#include "mhpc_control_map.h"

namespace mhpc_import_map {

enum Scope { STEPS_CONTROL = 0, STEPS_ALL = 1 };
enum Kind { X_NOM = 0, U_NOM, GAIN, ZGAIN, NKIND };
constexpr int NIN = 3;  // kinds with an input array (x_nom, u_nom, K)

MHPC_CTRL_HD inline bool scope_ok(int scope) { return scope == STEPS_CONTROL || scope == STEPS_ALL; }

// Columns of one window row of a kind, for rows of r.
MHPC_CTRL_HD inline int cols(int kind, int r) {
  return kind == X_NOM ? r : kind == GAIN ? 4 * r : kind == ZGAIN ? mhpc_ctrl::KW : 4;
}
// The dense block of one problem: what ld_* is at least, in elements.
MHPC_CTRL_HD inline long block(int kind, int r, int window) { return (long)window * cols(kind, r); }

// Phases whose knots are steps under a scope, and the state size of phase p.
MHPC_CTRL_HD inline int n_phases(int scope, int P, int n_wb) {
  return scope == STEPS_ALL ? P : mhpc_ctrl::n_phases(P, n_wb);
}
MHPC_CTRL_HD inline int phase_state(int p, int n_wb) { return p < n_wb ? 14 : 6; }

MHPC_CTRL_HD inline int n_steps(int scope, int P, int n_wb, const int* N) {
  int n = 0;
  for (int p = 0; p < n_phases(scope, P, n_wb); ++p) n += N[p] - 1;
  return n;
}
// Steps of a window of `window` rows from step `first` that exist.
MHPC_CTRL_HD inline int valid(int n_steps, int first, int window) {
  const int left = n_steps - first;
  return left < window ? (left < 0 ? 0 : left) : window;
}

struct Knot {
  int phase, k;  // the phase and the knot within it, k < N[phase] - 1
  int kk;        // the knot's index in the problem's packed arrays: ko[phase] + k
  int n;         // the state size of the phase
};
// Step j of a layout under a scope; false (and *o untouched) for a step outside [0, n_steps).
// Every phase is visited, so lanes with different steps run the same instructions.
MHPC_CTRL_HD inline bool knot_of(int scope, int P, int n_wb, const int* N, const int* ko, int j,
                                 Knot* o) {
  bool found = false;
  int off = 0;
  for (int p = 0; p < n_phases(scope, P, n_wb); ++p) {
    const int n = N[p] - 1;
    if (j >= off && j < off + n) {
      o->phase = p;
      o->k = j - off;
      o->kk = ko[p] + (j - off);
      o->n = phase_state(p, n_wb);
      found = true;
    }
    off += n;
  }
  return found;
}

// A layout as the map reads it, and the dimensions of the handle's arrays.
struct Lay {
  int P, n_wb;
  const int *N, *ko;
};
struct Dims {
  int NK, nslot;
};

struct Elem {
  int w, c;    // window row and column of the input element
  bool skip;   // past `valid`, or a column past the step's state size: not read, no destination
  int phase;   // the step's phase (valid only when !skip)
  size_t dst;  // element offset in traj (x_nom, u_nom) / K (gains)
};

// Input element e (0 <= e < block) of `kind` of problem b whose nominal slot is `slot`, for a
// window from step `first` with `nvalid` valid rows.
MHPC_CTRL_HD inline Elem elem(int scope, int kind, int r, const Lay& L, const Dims& D, int b,
                              int slot, int first, int nvalid, long e) {
  const int nc = cols(kind, r);
  Elem o;
  o.w = (int)(e / nc);
  o.c = (int)(e - (long)o.w * nc);
  o.skip = true;
  o.phase = 0;
  o.dst = 0;
  Knot q;
  if (o.w >= nvalid || !knot_of(scope, L.P, L.n_wb, L.N, L.ko, first + o.w, &q)) return o;
  o.phase = q.phase;
  if (kind == X_NOM) {
    if (o.c >= q.n) return o;
    o.dst = mhpc_ctrl::nom_off(D.NK, D.nslot, b, slot, q.kk) + o.c;
  } else if (kind == GAIN) {
    const int row = o.c / r, col = o.c - row * r;
    if (col >= q.n) return o;
    o.dst = mhpc_ctrl::gain_off(D.NK, b, q.kk) + row * q.n + col;
  } else if (kind == ZGAIN) {
    o.dst = mhpc_ctrl::gain_off(D.NK, b, q.kk) + o.c;
  } else {
    o.dst = mhpc_ctrl::nom_off(D.NK, D.nslot, b, slot, q.kk) + q.n + o.c;
  }
  o.skip = false;
  return o;
}

}  // namespace mhpc_import_map
