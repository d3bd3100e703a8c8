// Phase-buffer store of the receding-horizon loop (batch-wide save / load; the list-driven form
// is mhpc_tick.hip) and the exports of the nominal trajectories and the tracking references to
// the staging buffer.  Pure memory traffic, outside the solve.
#include <hip/hip_runtime.h>

#include "mhpc_device.h"
#include "mhpc_launch.h"

namespace MHPC_NS {

// ============================================================================================
// Phase buffers of the receding-horizon loop (MHPCLocomotion::update_problem,
// MHPCLocomotion.cpp:107-158): the reference keeps one N_TIMESTEPS_MAX-knot buffer per WB
// and per SRB phase slot (nominal x,u,y and cost-to-go) and rotates which buffer each phase
// uses.  store [B][spmax][nbk][SREC]: x,u,y (a traj record), K 56, du 4, G 14.  Phase p of a
// problem's layout lives in its buffer L.buf[p]; k_store_save runs with the layouts before
// an update, k_store_load with those after it.
// ============================================================================================
constexpr int SREC = kStoreRec;

__global__ void k_store_save(SolveParams sp, DevBufs d, real* store, int nbk, int spmax) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)sp.B * sp.NK) return;
  const int b = (int)(t / sp.NK), kk = (int)(t - (long)b * sp.NK);
  const Layout& L = d.grp[d.lid[b]].lay;  // the problem's layout (per lane: not a hot kernel)
  if (kk >= L.NK) return;
  int p = 0;
  while (p + 1 < L.P && kk >= L.ko[p + 1]) ++p;
  const int k = kk - L.ko[p];
  real* o = store + (((size_t)b * spmax + L.buf[p]) * nbk + k) * SREC;
  const real* r = traj_ptr(sp, d, b, d.st[b].nom_slot, kk);
  for (int i = 0; i < KS; ++i) o[i] = r[i];
  const size_t rec = (size_t)b * sp.NK + kk;
  for (int i = 0; i < 56; ++i) o[KS + i] = d.K[rec * 56 + i];
  for (int i = 0; i < 4; ++i) o[KS + 56 + i] = d.du[rec * 4 + i];
  for (int i = 0; i < 14; ++i) o[KS + 60 + i] = d.G[rec * 14 + i];
}

__global__ void k_store_load(SolveParams sp, DevBufs d, const real* store, int nbk, int spmax) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)sp.B * sp.NK) return;
  const int b = (int)(t / sp.NK), kk = (int)(t - (long)b * sp.NK);
  const Layout& L = d.grp[d.lid[b]].lay;  // the problem's layout (per lane: not a hot kernel)
  if (kk >= L.NK) return;
  int p = 0;
  while (p + 1 < L.P && kk >= L.ko[p + 1]) ++p;
  const int k = kk - L.ko[p];
  const real* o = store + (((size_t)b * spmax + L.buf[p]) * nbk + k) * SREC;
  real* r = traj_ptr(sp, d, b, 0, kk);  // k_init(warm = 0) sets nom_slot = 0
  for (int i = 0; i < KS; ++i) r[i] = o[i];
  if (k == L.N[p] - 1)  // u, y of the last knot are never rewritten by a sweep (B11): the
    for (int sl = 1; sl < sp.nslot; ++sl) {  // buffer's stale tail must follow any trial
      real* q = traj_ptr(sp, d, b, sl, kk);
      for (int i = 0; i < KS; ++i) q[i] = o[i];
    }
  const size_t rec = (size_t)b * sp.NK + kk;
  for (int i = 0; i < 56; ++i) d.K[rec * 56 + i] = o[KS + i];
  for (int i = 0; i < 4; ++i) d.du[rec * 4 + i] = o[KS + 56 + i];
  for (int i = 0; i < 14; ++i) d.G[rec * 14 + i] = o[KS + 60 + i];
}

hipError_t launch_store(const SolveParams& sp, const DevBufs& d, real* store, int nbk, int spmax,
                        int save, hipStream_t s) {
  const long n = (long)sp.B * sp.NK;
  if (save)
    hipLaunchKernelGGL(k_store_save, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, sp, d,
                       store, nbk, spmax);
  else
    hipLaunchKernelGGL(k_store_load, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, sp, d,
                       store, nbk, spmax);
  return hipGetLastError();
}

// Copy each problem's nominal trajectory (slot nom_slot) to a dense staging buffer.
__global__ void k_export(SolveParams sp, DevBufs d) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)sp.NK * KS;
  const int b = (int)(t / per);
  if (b >= sp.B) return;
  const long r = t - (long)b * per;
  const int nom = d.st[b].nom_slot;
  d.out[(size_t)b * per + r] = d.traj[(((size_t)b * sp.nslot + nom) * sp.NK) * KS + r];
}

// The tracking reference x of every knot of problems [b0, b0 + nb) into the staging buffer
// (mhpc_get_reference_problems): the reference's ms_ref_*[p][k].x as ReferenceGen::generate_ref
// leaves it (ReferenceGen.h:53-109), built by the helpers the cost kernels use.  Lane =
// (problem, knot of the knot stride); a record's entries past the phase's state size are zero.
__global__ void k_export_ref(SolveParams sp, DevBufs d, int b0, int nb) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)nb * sp.NK) return;
  const int b = b0 + (int)(t / sp.NK), kk = (int)(t % sp.NK);
  const Layout& L = d.grp[d.lid[b]].lay;  // the problem's layout (per lane: not a hot kernel)
  if (kk >= L.NK) return;
  int p = 0;
  while (p + 1 < L.P && kk >= L.ko[p + 1]) ++p;
  const bool wb = p < L.n_wb, last = kk - L.ko[p] == L.N[p] - 1;
  const Cmd cm = cmd_of(d, b);
  const real pos = d.refpos[(size_t)b * sp.NK + kk];
  real rx[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) rx[i] = real(0.0);
  if (wb) {
    if (last) wb_term_ref(cm, L.mode[p], pos, rx);
    else wb_run_ref(cm, pos, rx);
  } else {
    if (last) fb_term_ref(cm, pos, rx);
    else fb_run_ref(cm, pos, rx);
  }
  real* o = d.out + ((size_t)b * sp.NK + kk) * KS;
#pragma unroll
  for (int i = 0; i < 14; ++i) o[i] = rx[i];
}

// ---- launchers (called by mhpc_runtime.cpp) ---------------------------------------------
hipError_t launch_export(const SolveParams& sp, const DevBufs& d, hipStream_t s) {
  const long total = (long)sp.B * sp.NK * KS;
  hipLaunchKernelGGL(k_export, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sp, d);
  return hipGetLastError();
}
hipError_t launch_export_ref(const SolveParams& sp, const DevBufs& d, int b0, int nb, hipStream_t s) {
  const long total = (long)nb * sp.NK;
  hipLaunchKernelGGL(k_export_ref, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sp, d, b0,
                     nb);
  return hipGetLastError();
}

}  // namespace MHPC_NS
