// Device code of the control I/O entry points: measured states in, feedback controls out, both
// through arrays that stay on the device (mhpc_control_device, mhpc_set_x0_device; mhpc_control
// stages host arrays through the same kernel).
//
// k_control: one knot of forward_sweep_dynamics_only (SinglePhase.cpp:117-144),
// u = u_nom + K (x - x_nom), for every problem at a control step of its own (the step map is
// mhpc_step_map.h under STEPS_CONTROL).  Exactly serial_rollout's control law (mhpc_kernels.hip)
// at that knot with a run-time step size of +0: (u_nom[i] + eps du[i]) + fb_dot<n>(K row i, x,
// x_nom), the same fb_dot, so the result equals, bit for bit, what a policy rollout reports for
// the knot when the state is the one the rollout had there (tests/test_gpu_control.py).  Launched
// like the rollouts'
// lane_item(sp, d, 4, ...): blocks group by group, lane = (problem, control row i), the layout
// from the group record through scalar loads; the four lanes of a problem read its 56 contiguous
// gain words and each does one fb_dot.  The optional x_nom / u_nom / K outputs are stored by the
// same lanes, entry e of a problem's output by lane e mod 4.  The caller's arrays have an element
// type of their own (double or float), independent of the library's: inputs are rounded to real on
// the way in, outputs widened or rounded to nearest on the way out.
//
// k_x0_in: mhpc_set_x0 from a device array: rows of r at a stride of ld in the buffer's type to
// the handle's rows of 14 in real, an SRB-only problem's tail zero (pad_rows, mhpc_runtime.cpp).
//
// Launch-latency-sized, both: no LDS, no atomics, no scratch, every store a vector store, no
// index taken from array contents but the control step, which the host has checked against the
// same map (a lane whose step is outside its problem's steps stores nothing).
//
// In its own translation unit: the neighbours of the solve's kernels stay as they are (the fp32
// build's results are pinned to their code generation).
#include "mhpc_step_map.h"
#include "mhpc_device.h"
#include "mhpc_launch.h"

namespace MHPC_NS {

namespace sm = mhpc_steps;

static_assert(sm::KS == KS && sm::KW == 56 && sm::UW == 4 && sm::XW == 14,
              "mhpc_step_map.h restates the record widths of mhpc_solver.h");

template <class T>
struct ControlArgs {
  const int* step;  // [B] control step of each problem (null: step 0 for every problem)
  const T* x;       // measured states, row b at x + b * ldx (null only when u is null)
  T* u;             // controls, row b at u + b * ldu (null: not wanted)
  long ldx, ldu;
  T *x_nom, *u_nom, *K;  // dense [B][r], [B][4], [B][4][r]; each may be null
  int r;                 // row length of x / x_nom / K's rows: the handle's x0 row length
  real eps;              // the control's step size: +0 at run time, as k_policy_rollout's
};

// Control row i at one knot: the lines of serial_rollout's knot loop, with the state read from
// the caller's row.
template <int N, class T>
static __device__ __forceinline__ real control_row(const real* nk, const real* Kk, const real* duk,
                                                   const T* xr, real eps, int i) {
  real x[N];
#pragma unroll
  for (int c = 0; c < N; ++c) x[c] = (real)xr[c];
  const real fb = fb_dot<N>(Kk + i * N, x, nk);
  return (nk[N + i] + eps * duk[i]) + fb;
}

template <class T>
__global__ __launch_bounds__(64) void k_control(SolveParams sp, DevBufs d, ControlArgs<T> a) {
  int g, b, i;
  if (!lane_item(sp, d, 4, &g, &b, &i)) return;
  const Layout& L = layout_of(d, g);
  const int n = sm::control_state(L.n_wb);
  sm::Knot q;
  if (!sm::knot_of(sm::STEPS_CONTROL, L.P, L.n_wb, L.N, L.ko, a.step ? a.step[b] : 0, &q)) return;
  const real* nk = d.traj + sm::nom_off(sp.NK, sp.nslot, b, d.st[b].nom_slot, q.kk);
  const real* Kk = d.K + sm::gain_off(sp.NK, b, q.kk);
  if (a.u) {
    const real* duk = d.du + sm::du_off(sp.NK, b, q.kk);
    const T* xr = a.x + (size_t)b * a.ldx;
    const real u = n == 14 ? control_row<14>(nk, Kk, duk, xr, a.eps, i)
                           : control_row<6>(nk, Kk, duk, xr, a.eps, i);
    a.u[(size_t)b * a.ldu + i] = (T)u;
  }
  const int r = a.r;
  if (a.u_nom) a.u_nom[(size_t)b * 4 + i] = (T)nk[n + i];
  if (a.x_nom)
    for (int c = i; c < r; c += 4) a.x_nom[(size_t)b * r + c] = c < n ? (T)nk[c] : T(0);
  if (a.K)
    for (int e = i; e < 4 * r; e += 4) {  // entry e = (row, column) of the caller's [4][r] block
      const int row = e / r, col = e - row * r;
      a.K[(size_t)b * 4 * r + e] = col < n ? (T)Kk[row * n + col] : T(0);
    }
}

// Lane = (problem, entry of its device row of 14).
template <class T>
__global__ __launch_bounds__(256) void k_x0_in(SolveParams sp, DevBufs d, const T* x0, long ld) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)sp.B * 14) return;
  const int b = (int)(t / 14), c = (int)(t - (long)b * 14);
  const int n = sm::control_state(((CGroup*)d.grp + d.lid[b])->lay.n_wb);
  d.x0[t] = c < n ? (real)x0[(size_t)b * ld + c] : real(0.0);
}

static unsigned control_grid(const SolveParams& sp) {
  long n = 0;
  for (int g = 0; g < sp.ngrp; ++g) n += ((long)(sp.go[g + 1] - sp.go[g]) * 4 + 63) / 64;
  return (unsigned)n;
}

template <class T>
static hipError_t launch_control_t(const SolveParams& sp, const DevBufs& d, const int* step,
                                   const void* x, long ldx, void* u, long ldu, void* x_nom,
                                   void* u_nom, void* K, int r, hipStream_t s) {
  ControlArgs<T> a;
  a.step = step;
  a.x = (const T*)x;
  a.u = (T*)u;
  a.ldx = ldx;
  a.ldu = ldu;
  a.x_nom = (T*)x_nom;
  a.u_nom = (T*)u_nom;
  a.K = (T*)K;
  a.r = r;
  a.eps = 0;
  hipLaunchKernelGGL(k_control<T>, dim3(control_grid(sp)), dim3(64), 0, s, sp, d, a);
  return hipGetLastError();
}

hipError_t launch_control(const SolveParams& sp, const DevBufs& d, const int* step, const void* x,
                          long ldx, void* u, long ldu, void* x_nom, void* u_nom, void* K, int r,
                          int dtype, hipStream_t s) {
  return dtype == MHPC_DEV_F32
             ? launch_control_t<float>(sp, d, step, x, ldx, u, ldu, x_nom, u_nom, K, r, s)
             : launch_control_t<double>(sp, d, step, x, ldx, u, ldu, x_nom, u_nom, K, r, s);
}

hipError_t launch_x0_in(const SolveParams& sp, const DevBufs& d, const void* x0, long ld, int dtype,
                        hipStream_t s) {
  const dim3 grid((unsigned)(((long)sp.B * 14 + 255) / 256));
  if (dtype == MHPC_DEV_F32)
    hipLaunchKernelGGL(k_x0_in<float>, grid, dim3(256), 0, s, sp, d, (const float*)x0, ld);
  else
    hipLaunchKernelGGL(k_x0_in<double>, grid, dim3(256), 0, s, sp, d, (const double*)x0, ld);
  return hipGetLastError();
}

}  // namespace MHPC_NS
