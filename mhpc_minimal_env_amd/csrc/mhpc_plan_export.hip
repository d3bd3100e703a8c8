// Device code of the plan export entry points: windows of a problem's policy and the results of
// its last solve into device arrays of the caller's (mhpc_export_plan_device,
// mhpc_export_results_device).
//
// k_plan_export: for each listed problem, W consecutive control steps from a first step of its
// own -- x_nom, u_nom, K, du, Vx, y and the step's mode -- into the caller's [n][W][c] blocks.
// Pure memory traffic, list-driven: a block per (listed problem, chunk of PW_CH window rows), so
// no block spans two problems and device work follows the list, never the batch.  The problem is
// block-uniform (window_block, mhpc_plan_window.h, shared with the import): its list entry, first
// step, group record d.grp[d.lid[b]] and nominal slot are read through scalar loads.  Per wanted
// array the block's lanes stride over the chunk's output elements, consecutive lanes storing
// consecutive elements (whole lines per store instruction);
// the source of each element is what mhpc_step_map.h names, contiguous inside a phase too (K: 4 n
// of a knot's 56 words, knots adjacent).  The map's knot_of visits every control phase, so lanes
// of different rows run the same instructions.  Rows past `valid` and columns past the state size
// are stored as +0; nothing is stored outside a listed problem's [W][c] block.  The only
// arithmetic is the element-type conversion of the control I/O (mhpc_control.hip): widened for a
// double array, rounded to nearest for a float array.
//
// k_results_export: lane = (listed problem, output word) of J, dV_exp, viol, V[P], dV[P], status;
// each lane reads the one ProbState field it stores.
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

static_assert(sm::KS == KS && sm::KW == 56 && sm::UW == 4 && sm::GW == 14,
              "mhpc_step_map.h restates the record widths of mhpc_solver.h");

template <class T>
struct PlanArgs {
  const int* list;   // [n] listed problems (null: problem i)
  const int* first;  // [n] first step of each (null: 0)
  int window, r;
  T *x_nom, *u_nom, *K, *du, *Vx, *y;  // each may be null
  long ld[sm::NOUT];                   // elements between two listed problems' blocks
  int32_t *mode, *valid;
};

// One kind's share of a block: output elements [w0, w1) x cols of the block's listed problem.
template <int KIND, class T, class S>
static __device__ __forceinline__ void export_kind(T* out, long ld, const S* src, int r,
                                                   const WindowBlock& k) {
  const int nc = sm::cols(KIND, r);
  T* o = out + (size_t)k.i * (size_t)ld;
  for (long e = (long)k.w0 * nc + threadIdx.x; e < (long)k.w1 * nc; e += PW_NT) {
    const sm::Elem q =
        sm::elem(sm::STEPS_CONTROL, KIND, r, k.L, k.D, k.b, k.slot, k.first, k.nvalid, e);
    o[e] = q.skip ? T(0) : (T)src[q.off];
  }
}

template <class T>
__global__ __launch_bounds__(PW_NT) void k_plan_export(SolveParams sp, DevBufs d, PlanArgs<T> a,
                                                       int nch) {
  const WindowBlock k = window_block(sp, d, a.list, a.first, a.window, sm::STEPS_CONTROL, nch);
  if (a.valid && k.w0 == 0 && threadIdx.x == 0) a.valid[k.i] = k.nvalid;
  const int r = a.r;
  if (a.x_nom) export_kind<sm::X_NOM>(a.x_nom, a.ld[sm::X_NOM], d.traj, r, k);
  if (a.u_nom) export_kind<sm::U_NOM>(a.u_nom, a.ld[sm::U_NOM], d.traj, r, k);
  if (a.K) export_kind<sm::GAIN>(a.K, a.ld[sm::GAIN], d.K, r, k);
  if (a.du) export_kind<sm::DU>(a.du, a.ld[sm::DU], d.du, r, k);
  if (a.Vx) export_kind<sm::VX>(a.Vx, a.ld[sm::VX], d.G, r, k);
  if (a.y) export_kind<sm::Y>(a.y, a.ld[sm::Y], d.traj, r, k);
  if (a.mode) export_kind<sm::MODE>(a.mode, a.ld[sm::MODE], k.mode, r, k);
}

template <class T>
struct ResultArgs {
  const int* list;  // [n] listed problems (null: problem i)
  int n, P;         // listed problems; row length of V_phase / dV_phase (the handle's most phases)
  T *J, *dV_exp, *viol, *V, *dV;  // each may be null
  int32_t* status;
};

// Word wd of a problem's results: 0 J, 1 dV_exp, 2 viol, 3 status, then V[P], then dV[P].
template <class T>
__global__ __launch_bounds__(256) void k_results_export(DevBufs d, ResultArgs<T> a) {
  const int nw = 4 + 2 * a.P;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)a.n * nw) return;
  const int i = (int)(t / nw), wd = (int)(t - (long)i * nw);
  const int b = a.list ? a.list[i] : i;
  const ProbState* st = d.st + b;
  if (wd == 0) {
    if (a.J) a.J[i] = (T)st->J;
  } else if (wd == 1) {
    if (a.dV_exp) a.dV_exp[i] = (T)st->dV_exp;
  } else if (wd == 2) {
    if (a.viol) a.viol[i] = (T)st->viol;
  } else if (wd == 3) {
    if (a.status) a.status[i] = st->status;
  } else {
    const int p = (wd - 4) % a.P;
    T* o = wd - 4 < a.P ? a.V : a.dV;
    if (!o) return;
    const int P = ((CGroup*)d.grp + d.lid[b])->lay.P;  // zero past the problem's own phases
    const acc* s = wd - 4 < a.P ? st->V : st->dV;
    o[(size_t)i * a.P + p] = p < P ? (T)s[p] : T(0);
  }
}

template <class T>
static hipError_t launch_plan_export_t(const SolveParams& sp, const DevBufs& d, int n,
                                       const int* list, const int* first, int window, int r,
                                       void* const* arrays, const long* ld, int32_t* valid,
                                       hipStream_t s) {
  PlanArgs<T> a;
  a.list = list;
  a.first = first;
  a.window = window;
  a.r = r;
  a.x_nom = (T*)arrays[sm::X_NOM];
  a.u_nom = (T*)arrays[sm::U_NOM];
  a.K = (T*)arrays[sm::GAIN];
  a.du = (T*)arrays[sm::DU];
  a.Vx = (T*)arrays[sm::VX];
  a.y = (T*)arrays[sm::Y];
  a.mode = (int32_t*)arrays[sm::MODE];
  a.valid = valid;
  for (int k = 0; k < sm::NOUT; ++k) a.ld[k] = ld[k];
  const int nch = window_chunks(window);
  hipLaunchKernelGGL(k_plan_export<T>, dim3((unsigned)n * nch), dim3(PW_NT), 0, s, sp, d, a, nch);
  return hipGetLastError();
}

hipError_t launch_plan_export(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                              const int* first, int window, int r, void* const* arrays,
                              const long* ld, int32_t* valid, int dtype, hipStream_t s) {
  return dtype == MHPC_DEV_F32
             ? launch_plan_export_t<float>(sp, d, n, list, first, window, r, arrays, ld, valid, s)
             : launch_plan_export_t<double>(sp, d, n, list, first, window, r, arrays, ld, valid, s);
}

template <class T>
static hipError_t launch_results_export_t(const DevBufs& d, int n, const int* list, int P,
                                          void* const* arrays, int32_t* status, hipStream_t s) {
  ResultArgs<T> a;
  a.list = list;
  a.n = n;
  a.P = P;
  a.J = (T*)arrays[0];
  a.dV_exp = (T*)arrays[1];
  a.viol = (T*)arrays[2];
  a.V = (T*)arrays[3];
  a.dV = (T*)arrays[4];
  a.status = status;
  const long total = (long)n * (4 + 2 * P);
  hipLaunchKernelGGL(k_results_export<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d,
                     a);
  return hipGetLastError();
}

hipError_t launch_results_export(const DevBufs& d, int n, const int* list, int P,
                                 void* const* arrays, int32_t* status, int dtype, hipStream_t s) {
  return dtype == MHPC_DEV_F32 ? launch_results_export_t<float>(d, n, list, P, arrays, status, s)
                               : launch_results_export_t<double>(d, n, list, P, arrays, status, s);
}

}  // namespace MHPC_NS
