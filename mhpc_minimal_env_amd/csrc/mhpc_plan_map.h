// The window map of mhpc_export_plan_device: which element of a problem's packed arrays an
// element of a caller's [W][c] block comes from.
//
// A window is W consecutive control steps of one problem from a first step on (the steps of
// mhpc_control_map.h: a window runs across phase boundaries exactly as consecutive steps do, a
// phase's last knot is never a step).  Its `valid` rows exist; the rows past them, and the
// columns past the problem's state size n in rows of the handle's x0 row length r, are +0.
// Seven kinds of output share the map:
//   x_nom [W][r]      traj record of the knot, entries 0..n          (nominal slot)
//   u_nom [W][4]      traj record, entries n..n+4
//   y     [W][4]      traj record, entries n+4..n+8
//   K     [W][4][r]   the 4 n dense words of the knot's 56, row i at i n
//   du    [W][4]      as stored
//   Vx    [W][r]      the first n of G's 14
//   mode  [W]         the mode of the step's phase: the source is the phase index
//
// The kernel (mhpc_plan_export.hip), the runtime's validation (mhpc_runtime.cpp) and the host
// check (tests/native/plan_map_hostcheck.cpp) run the same code; everything here is plain integer
// arithmetic on the layout, no index comes from array contents.
#pragma once
#include "mhpc_control_map.h"

namespace mhpc_plan_map {

constexpr int GW = 14;  // a knot's row of G (mhpc_plan_export.hip asserts the widths)
enum Kind { X_NOM = 0, U_NOM, GAIN, DU, VX, Y, MODE, NKIND };

// Columns of one window row of an output kind, for rows of r.
MHPC_CTRL_HD inline int cols(int kind, int r) {
  return kind == X_NOM || kind == VX ? r : kind == GAIN ? 4 * r : kind == MODE ? 1 : 4;
}
// The dense block of one problem: what ld_* is at least, in elements.
MHPC_CTRL_HD inline long block(int kind, int r, int window) { return (long)window * cols(kind, r); }

// Steps of a window of `window` rows from step `first` that exist (first in 0..n_steps-1).
MHPC_CTRL_HD inline int valid(int n_steps, int first, int window) {
  const int left = n_steps - first;
  return left < window ? (left < 0 ? 0 : left) : window;
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
  int w, c;    // window row and column of the output element
  bool zero;   // past `valid`, or a column past the state size: +0, no source
  int phase;   // the step's phase (valid only when !zero)
  size_t src;  // element offset in traj (x_nom, u_nom, y) / K / du / G; the phase for mode
};

// Output element e (0 <= e < block) of `kind` of problem b whose nominal slot is `slot`, for a
// window from step `first` with `nvalid` valid rows.
MHPC_CTRL_HD inline Elem elem(int kind, int r, const Lay& L, const Dims& D, int b, int slot,
                              int first, int nvalid, long e) {
  const int nc = cols(kind, r);
  Elem o;
  o.w = (int)(e / nc);
  o.c = (int)(e - (long)o.w * nc);
  o.zero = true;
  o.phase = 0;
  o.src = 0;
  mhpc_ctrl::Knot q;
  if (o.w >= nvalid || !mhpc_ctrl::knot_of(L.P, L.n_wb, L.N, L.ko, first + o.w, &q)) return o;
  const int n = mhpc_ctrl::state_size(L.n_wb);
  o.phase = q.phase;
  if (kind == X_NOM || kind == VX) {
    if (o.c >= n) return o;
    o.src = kind == X_NOM ? mhpc_ctrl::nom_off(D.NK, D.nslot, b, slot, q.kk) + o.c
                          : ((size_t)b * D.NK + q.kk) * GW + o.c;
  } else if (kind == GAIN) {
    const int row = o.c / r, col = o.c - row * r;
    if (col >= n) return o;
    o.src = mhpc_ctrl::gain_off(D.NK, b, q.kk) + row * n + col;
  } else if (kind == U_NOM || kind == Y) {
    o.src = mhpc_ctrl::nom_off(D.NK, D.nslot, b, slot, q.kk) + n + (kind == Y ? 4 : 0) + o.c;
  } else if (kind == DU) {
    o.src = mhpc_ctrl::du_off(D.NK, b, q.kk) + o.c;
  } else {
    o.src = (size_t)q.phase;
  }
  o.zero = false;
  return o;
}

}  // namespace mhpc_plan_map
