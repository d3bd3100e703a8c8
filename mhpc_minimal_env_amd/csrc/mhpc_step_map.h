// The step-and-window map of the device-resident I/O (mhpc_control / mhpc_control_device,
// mhpc_export_plan_device, mhpc_import_plan / mhpc_import_plan_device): which knot of a problem's
// packed arrays a step names, and which element of those arrays an element of a caller's [W][c]
// window block comes from or goes to.
//
// Steps.  A problem's policy is addressed by an integer step, never by a time (a time divided by
// dt at a knot boundary rounds either way).  Two step maps (`scope`):
//   STEPS_CONTROL  the control steps: the whole-body phases of a problem that has any -- an SRB
//                  phase's control is a ground-reaction force, nothing to apply to the robot -- and
//                  all phases of an SRB-only problem.  Every step has the problem's one state size
//                  (14 or 6), so a window that the export wrote goes back element for element.
//   STEPS_ALL      every phase of the problem in order.  The state size is the phase's: 14 in a
//                  whole-body phase, 6 in an SRB phase.
// Phase p contributes N[p] - 1 steps (its last knot has no control and is never a step), so step j
// is knot k = j - off_p of the phase p with off_p <= j < off_p + N[p] - 1, off_p = sum over q < p
// of (N[q] - 1).  The knot's index in the packed arrays is ko[p] + k with the layout's own ko (the
// layout of the problem as mhpc_update_problem(s) left it), and its nominal record lies in the
// trajectory slot the problem's state names (nom_slot).
//
// Windows.  A window is W consecutive steps of one problem from a first step on: it runs across
// phase boundaries exactly as consecutive steps do.  Its `valid` rows exist.  The rows past them,
// and in rows of the handle's x0 row length r the columns past the step's state size n, are
// skipped: the export stores them as +0, the import does not read them.  The kinds of block:
//   x_nom [W][r]      traj record of the knot, entries 0..n          (nominal slot)
//   u_nom [W][4]      traj record, entries n..n+4
//   K     [W][4][r]   the 4 n dense words of the knot's 56, row i at i n
//   du    [W][4]      as stored                                      (export only)
//   Vx    [W][r]      the first n of G's 14                          (export only)
//   y     [W][4]      traj record, entries n+4..n+8                  (export only)
//   mode  [W]         the mode of the step's phase: the offset is the phase index (export only)
//   zero gains [W][56] (no caller array) all 56 gain words of the knot: an import without K
// The export-only kinds are never a destination: the import has no array for them (NIN).
//
// The kernels (mhpc_control.hip, mhpc_plan_export.hip, mhpc_plan_import.hip), the runtime's
// validation (mhpc_runtime.cpp) and the host check (tests/native/step_map_hostcheck.cpp) run the
// same code; everything here is plain integer arithmetic on the layout, no index comes from array
// contents.  The control kernel and the export pass the constant STEPS_CONTROL, so the scope folds
// away in their code.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MHPC_MAP_HD __host__ __device__
#else
#define MHPC_MAP_HD
#endif

namespace mhpc_steps {

// record widths of mhpc_solver.h (the three .hip files assert that they agree)
constexpr int KS = 24, KW = 56, UW = 4, XW = 14, GW = 14;

enum Scope { STEPS_CONTROL = 0, STEPS_ALL = 1 };
// The seven export kinds first (they index the export's arrays [NOUT] and ld [NOUT]), of which the
// first three have an input array of the import's (arrays [NIN] and ld [NIN]).
enum Kind { X_NOM = 0, U_NOM, GAIN, DU, VX, Y, MODE, ZGAIN, NKIND };
constexpr int NIN = 3, NOUT = 7;

MHPC_MAP_HD inline bool scope_ok(int scope) { return scope == STEPS_CONTROL || scope == STEPS_ALL; }

// Phases whose knots are steps under a scope, and the state size of phase p.
MHPC_MAP_HD inline int n_phases(int scope, int P, int n_wb) {
  return scope == STEPS_ALL ? P : n_wb > 0 ? n_wb : P;
}
MHPC_MAP_HD inline int phase_state(int p, int n_wb) { return p < n_wb ? 14 : 6; }
// The one state size of a problem's control steps: phase 0's.
MHPC_MAP_HD inline int control_state(int n_wb) { return phase_state(0, n_wb); }

MHPC_MAP_HD inline int n_steps(int scope, int P, int n_wb, const int* N) {
  int n = 0;
  for (int p = 0; p < n_phases(scope, P, n_wb); ++p) n += N[p] - 1;
  return n;
}
// Steps of a window of `window` rows from step `first` that exist.
MHPC_MAP_HD inline int valid(int n_steps, int first, int window) {
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
MHPC_MAP_HD inline bool knot_of(int scope, int P, int n_wb, const int* N, const int* ko, int j,
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

// Element offsets of knot kk of problem b: its record in trajectory slot `slot` of traj
// [B][nslot][NK][KS] (x first, then u, then y), its gain block in K [B][NK][56] (4 rows of the
// state size, dense), its feed-forward row in du [B][NK][4] and its row of G [B][NK][14].
MHPC_MAP_HD inline size_t nom_off(int NK, int nslot, int b, int slot, int kk) {
  return (((size_t)b * nslot + slot) * NK + kk) * KS;
}
MHPC_MAP_HD inline size_t gain_off(int NK, int b, int kk) { return ((size_t)b * NK + kk) * KW; }
MHPC_MAP_HD inline size_t du_off(int NK, int b, int kk) { return ((size_t)b * NK + kk) * UW; }
MHPC_MAP_HD inline size_t g_off(int NK, int b, int kk) { return ((size_t)b * NK + kk) * GW; }

// A layout as the map reads it, and the dimensions of the handle's arrays.
struct Lay {
  int P, n_wb;
  const int *N, *ko;
};
struct Dims {
  int NK, nslot;
};

// Columns of one window row of a kind, for rows of r.
MHPC_MAP_HD inline int cols(int kind, int r) {
  return kind == X_NOM || kind == VX ? r
         : kind == GAIN              ? 4 * r
         : kind == MODE              ? 1
         : kind == ZGAIN             ? KW
                                     : 4;
}
// The dense block of one problem: what ld_* is at least, in elements.
MHPC_MAP_HD inline long block(int kind, int r, int window) { return (long)window * cols(kind, r); }

struct Elem {
  int w, c;    // window row and column of the caller's element
  bool skip;   // past `valid`, or a column past the step's state size: +0 out, not read in
  int phase;   // the step's phase (valid only when !skip)
  size_t off;  // element offset in traj (x_nom, u_nom, y) / K (gains) / du / G; the phase for mode
};

// Column c of a window row of `kind` whose step is knot q, of problem b whose nominal slot is
// `slot`: false for a column past the knot's state size, else true and *off the element's offset.
MHPC_MAP_HD inline bool knot_elem(int kind, int r, const Dims& D, int b, int slot, const Knot& q,
                                  int c, size_t* off) {
  if (kind == X_NOM || kind == VX) {
    if (c >= q.n) return false;
    *off = (kind == X_NOM ? nom_off(D.NK, D.nslot, b, slot, q.kk) : g_off(D.NK, b, q.kk)) + c;
  } else if (kind == GAIN) {
    const int row = c / r, col = c - row * r;
    if (col >= q.n) return false;
    *off = gain_off(D.NK, b, q.kk) + row * q.n + col;
  } else if (kind == U_NOM || kind == Y) {
    *off = nom_off(D.NK, D.nslot, b, slot, q.kk) + q.n + (kind == Y ? 4 : 0) + c;
  } else if (kind == DU) {
    *off = du_off(D.NK, b, q.kk) + c;
  } else if (kind == ZGAIN) {
    *off = gain_off(D.NK, b, q.kk) + c;
  } else {
    *off = (size_t)q.phase;
  }
  return true;
}

// Element e (0 <= e < block) of `kind` of problem b whose nominal slot is `slot`, for a window
// from step `first` with `nvalid` valid rows.
MHPC_MAP_HD inline Elem elem(int scope, int kind, int r, const Lay& L, const Dims& D, int b,
                             int slot, int first, int nvalid, long e) {
  const int nc = cols(kind, r);
  Elem o;
  o.w = (int)(e / nc);
  o.c = (int)(e - (long)o.w * nc);
  o.skip = true;
  o.phase = 0;
  o.off = 0;
  Knot q;
  if (o.w >= nvalid || !knot_of(scope, L.P, L.n_wb, L.N, L.ko, first + o.w, &q)) return o;
  o.phase = q.phase;
  size_t off;
  if (!knot_elem(kind, r, D, b, slot, q, o.c, &off)) return o;
  o.off = off;
  o.skip = false;
  return o;
}

}  // namespace mhpc_steps
