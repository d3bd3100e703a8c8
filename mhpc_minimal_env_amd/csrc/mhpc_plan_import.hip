// Device code of the plan import entry point: windows of a guessed policy from device arrays of
// the caller's into the packed records of the listed problems (mhpc_import_plan_device).
//
// k_plan_import mirrors k_plan_export (mhpc_plan_export.hip) in the other direction: for each
// listed problem, W consecutive steps from a first step of its own -- u_nom, and optionally x_nom
// and K -- out of the caller's [n][W][c] blocks.  Pure memory traffic, list-driven: a block per
// (listed problem, chunk of PW_CH window rows), so no block spans two problems and device work
// follows the list, never the batch.  The problem is block-uniform (window_block,
// mhpc_plan_window.h, shared with the export): its list entry, first step, group record
// d.grp[d.lid[b]] and nominal slot are read through scalar loads.  Per given array
// the block's lanes stride over the chunk's input elements, consecutive lanes loading consecutive
// elements (whole lines per load instruction); the destination of each element is what
// mhpc_step_map.h names, contiguous inside a phase too.  The map's knot_of visits every phase of
// the scope, so lanes of different rows run the same instructions.  Rows past `valid` and columns
// past the step's state size are not read; nothing is stored outside the named entries of a
// listed problem's window knots (never y, du, G, another trajectory slot, the partials or the
// problem's state).  Without K the 56 gain words of every window knot are stored as +0.  The only
// arithmetic is the element-type conversion of the control I/O (mhpc_control.hip): widened from a
// float array, rounded to nearest from a double array into an fp32 handle.
//
// No LDS, no atomics, no scratch, plain C++ stores; 64-bit offsets; the only indices taken from
// memory are the list entry and the first step, both checked by the host against the same map,
// and the nominal slot, which the host never lets leave 0..nslot-1.
//
// In its own translation unit: the neighbours of the solve's kernels stay as they are (the fp32
// build's results are pinned to their code generation).
#include "mhpc_plan_window.h"
#include "mhpc_launch.h"

namespace MHPC_NS {

static_assert(sm::KS == KS && sm::KW == 56 && sm::UW == 4,
              "mhpc_step_map.h restates the record widths of mhpc_solver.h");

template <class T>
struct ImportArgs {
  const int* list;   // [n] listed problems (null: problem i)
  const int* first;  // [n] first step of each (null: 0)
  int window, r, scope;
  const T *x_nom, *u_nom, *K;  // x_nom and K may be null (together)
  long ld[sm::NIN];            // elements between two listed problems' blocks
};

// One kind's share of a block: input elements [w0, w1) x cols of the block's listed problem.
template <int KIND, class T>
static __device__ __forceinline__ void import_kind(const T* in, long ld, real* dst, int scope,
                                                   int r, const WindowBlock& k) {
  const int nc = sm::cols(KIND, r);
  const T* src = KIND == sm::ZGAIN ? nullptr : in + (size_t)k.i * (size_t)ld;
  for (long e = (long)k.w0 * nc + threadIdx.x; e < (long)k.w1 * nc; e += PW_NT) {
    const sm::Elem q = sm::elem(scope, KIND, r, k.L, k.D, k.b, k.slot, k.first, k.nvalid, e);
    if (q.skip) continue;
    if constexpr (KIND == sm::ZGAIN)
      dst[q.off] = real(0);
    else
      dst[q.off] = (real)src[e];
  }
}

template <class T>
__global__ __launch_bounds__(PW_NT) void k_plan_import(SolveParams sp, DevBufs d, ImportArgs<T> a,
                                                       int nch) {
  const int scope = a.scope, r = a.r;
  const WindowBlock k = window_block(sp, d, a.list, a.first, a.window, scope, nch);
  import_kind<sm::U_NOM>(a.u_nom, a.ld[sm::U_NOM], d.traj, scope, r, k);
  if (a.K) {
    import_kind<sm::X_NOM>(a.x_nom, a.ld[sm::X_NOM], d.traj, scope, r, k);
    import_kind<sm::GAIN>(a.K, a.ld[sm::GAIN], d.K, scope, r, k);
  } else {
    import_kind<sm::ZGAIN>((const T*)nullptr, 0, d.K, scope, r, k);
  }
}

template <class T>
static hipError_t launch_plan_import_t(const SolveParams& sp, const DevBufs& d, int n,
                                       const int* list, const int* first, int window, int scope,
                                       int r, const void* const* arrays, const long* ld,
                                       hipStream_t s) {
  ImportArgs<T> a;
  a.list = list;
  a.first = first;
  a.window = window;
  a.r = r;
  a.scope = scope;
  a.x_nom = (const T*)arrays[sm::X_NOM];
  a.u_nom = (const T*)arrays[sm::U_NOM];
  a.K = (const T*)arrays[sm::GAIN];
  for (int k = 0; k < sm::NIN; ++k) a.ld[k] = ld[k];
  const int nch = window_chunks(window);
  hipLaunchKernelGGL(k_plan_import<T>, dim3((unsigned)n * nch), dim3(PW_NT), 0, s, sp, d, a, nch);
  return hipGetLastError();
}

hipError_t launch_plan_import(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                              const int* first, int window, int scope, int r,
                              const void* const* arrays, const long* ld, int dtype,
                              hipStream_t s) {
  return dtype == MHPC_DEV_F32
             ? launch_plan_import_t<float>(sp, d, n, list, first, window, scope, r, arrays, ld, s)
             : launch_plan_import_t<double>(sp, d, n, list, first, window, scope, r, arrays, ld, s);
}

}  // namespace MHPC_NS
