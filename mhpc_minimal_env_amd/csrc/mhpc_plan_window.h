// The device-side piece k_plan_export (mhpc_plan_export.hip) and k_plan_import
// (mhpc_plan_import.hip) share: a block serves one chunk of PW_CH window rows of one listed
// problem, and what it knows about that problem before it touches a caller's array.
#pragma once
#include "mhpc_device.h"
#include "mhpc_step_map.h"

namespace MHPC_NS {

namespace sm = mhpc_steps;

constexpr int PW_CH = 16;  // window rows a block serves (K: 16 rows of 4 r elements, 3.5 passes)
constexpr int PW_NT = 256;

// Blocks a listed problem's window takes: the launchers' grid is n * window_chunks(window).
inline int window_chunks(int window) { return (window + PW_CH - 1) / PW_CH; }

// The problem is block-uniform: its list entry, first step, group record d.grp[d.lid[b]] and
// nominal slot are read through scalar loads.
struct WindowBlock {
  int i, b;      // position in the list, and the problem (list null: problem i)
  int first;     // first step of the window (first null: 0)
  int slot;      // the problem's nominal trajectory slot
  int nvalid;    // rows of the window that are steps of the problem under the scope
  int w0, w1;    // the block's rows [w0, w1)
  sm::Lay L;
  sm::Dims D;
  const int* mode;  // the layout's mode of each phase
};
static __device__ __forceinline__ WindowBlock window_block(const SolveParams& sp, const DevBufs& d,
                                                           const int* list, const int* first,
                                                           int window, int scope, int nch) {
  WindowBlock k;
  k.i = blockIdx.x / nch;
  k.w0 = (int)(blockIdx.x % nch) * PW_CH;
  k.w1 = min(k.w0 + PW_CH, window);
  k.b = list ? list[k.i] : k.i;
  k.first = first ? first[k.i] : 0;
  const Layout& Ly = layout_of(d, d.lid[k.b]);
  k.L = {Ly.P, Ly.n_wb, Ly.N, Ly.ko};
  k.D = {sp.NK, sp.nslot};
  k.slot = d.st[k.b].nom_slot;
  k.nvalid = sm::valid(sm::n_steps(scope, k.L.P, k.L.n_wb, k.L.N), k.first, window);
  k.mode = Ly.mode;
  return k;
}

}  // namespace MHPC_NS
