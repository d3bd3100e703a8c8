// Device code of mhpc_tick_problems that the batch-wide update has no list-driven form of: the
// phase-buffer save / load of the listed problems (k_store_save / k_store_load of
// mhpc_store.hip walk B * NK threads) and the gather of their status words.  Every other kernel
// of a tick is one of the solve's own, launched over the tick's scope.
//
// Pure memory traffic, list-driven: device work is proportional to the number of listed problems,
// never to the batch.  No LDS, no atomics, no index taken from array contents but the problem's
// nominal slot, which the host never lets leave 0..nslot-1; every store is a vector store.
//
// In its own translation unit: the neighbours of the solve's kernels stay as they are (the fp32
// build's results are pinned to their code generation).
#include "mhpc_launch.h"

namespace MHPC_NS {

// store [B][spmax][nbk][kStoreRec]: x,u,y (a traj record, KS), K 56, du 4, G 14 per knot; phase p
// of a problem's layout lives in its buffer L.buf[p] (mhpc_store.hip, k_store_save).
constexpr int SREC = kStoreRec;
constexpr int TL_CH = 64;  // knots of the stride a block serves (k_reset_list's chunk)

// A block per (listed problem, chunk of TL_CH knots of the stride).  The chunk's knots of one
// phase are contiguous in that phase's buffer, SREC reals a knot, so the block's lanes stride over
// those elements (whole lines per wave on the store's side) and gather (SAVE) or scatter (load)
// the traj record, K, du and G of the knot each element belongs to -- runs of 24, 56, 4 and 14
// reals on the arrays' side, where k_store_save / k_store_load make 98 strided accesses a thread.
// SAVE reads the problem's nominal slot and runs with the layouts before a commit; the load runs
// with those after it, behind k_init(warm = 0), which set nom_slot = 0: it writes slot 0 and, at a
// phase's last knot, the record into every other slot (u, y there are never rewritten by a sweep,
// quirk B11: the buffer's stale tail must follow any trial).  The layout is the problem's own,
// d.grp[d.lid[b]], block-uniform.
template <bool SAVE>
__global__ __launch_bounds__(256) void k_store_list(SolveParams sp, DevBufs d, const int* list,
                                                    int nch, real* store, int nbk, int spmax) {
  const int b = list[blockIdx.x / nch], i0 = (int)(blockIdx.x % nch) * TL_CH, t = threadIdx.x;
  const Layout& L = d.grp[d.lid[b]].lay;
  const int i1 = min(i0 + TL_CH, L.NK);
  if (i0 >= i1) return;
  const int slot = SAVE ? d.st[b].nom_slot : 0;
  real* tr = d.traj + ((size_t)b * sp.nslot + slot) * sp.NK * KS;
  const size_t rec0 = (size_t)b * sp.NK;
  for (int p = 0; p < L.P; ++p) {
    const int k0 = max(i0, L.ko[p]), k1 = min(i1, L.ko[p] + L.N[p]);  // the chunk's knots of phase p
    if (k0 >= k1) continue;
    real* o = store + (((size_t)b * spmax + L.buf[p]) * nbk + (k0 - L.ko[p])) * SREC;
    for (int e = t; e < (k1 - k0) * SREC; e += 256) {
      const int j = e / SREC, f = e - j * SREC;
      const size_t kk = (size_t)(k0 + j);
      real* a = f < KS        ? tr + kk * KS + f
                : f < KS + 56 ? d.K + (rec0 + kk) * 56 + (f - KS)
                : f < KS + 60 ? d.du + (rec0 + kk) * 4 + (f - KS - 56)
                              : d.G + (rec0 + kk) * 14 + (f - KS - 60);
      if (SAVE)
        o[e] = *a;
      else
        *a = o[e];
    }
    if (!SAVE && k1 == L.ko[p] + L.N[p]) {  // the phase's last knot is this chunk's
      const real* ol = o + (size_t)(k1 - 1 - k0) * SREC;
      for (int e = t; e < (sp.nslot - 1) * KS; e += 256) {
        const int sl = 1 + e / KS, f = e % KS;
        d.traj[(((size_t)b * sp.nslot + sl) * sp.NK + (k1 - 1)) * KS + f] = ol[f];
      }
    }
  }
}

// status [n] in list order <- the listed problems' status words (mhpc_solve copies the whole
// ProbState array to read one word a problem).
__global__ __launch_bounds__(64) void k_status_list(DevBufs d, int n, const int* list,
                                                    int32_t* status) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) status[i] = d.st[list[i]].status;
}

hipError_t launch_store_list(const SolveParams& sp, const DevBufs& d, int n, const int* list,
                             real* store, int nbk, int spmax, int save, hipStream_t s) {
  const int nch = (sp.NK + TL_CH - 1) / TL_CH;
  if (save)
    hipLaunchKernelGGL(k_store_list<true>, dim3((unsigned)n * nch), dim3(256), 0, s, sp, d, list, nch,
                       store, nbk, spmax);
  else
    hipLaunchKernelGGL(k_store_list<false>, dim3((unsigned)n * nch), dim3(256), 0, s, sp, d, list,
                       nch, store, nbk, spmax);
  return hipGetLastError();
}

hipError_t launch_status_list(const DevBufs& d, int n, const int* list, int32_t* status,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_status_list, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d, n, list,
                     status);
  return hipGetLastError();
}

}  // namespace MHPC_NS
