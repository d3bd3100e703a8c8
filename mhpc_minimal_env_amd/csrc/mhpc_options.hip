// Device code of mhpc_set_option_sets (and of mhpc_copy_problems' option hand-over): the listed
// problems' entries of the per-problem option index, and the option fields a solve rewrites.
//
// Giving a problem an option record is the reference's `_option = o` on that controller: the fields
// a solve only reads (budgets, thresholds, gamma, the update factors, AL_active) live in the table
// DevBufs::opt and take effect through oid[b] at the problem's next solve; ReB_active and
// update_penalty are rewritten inside a solve (MultiPhaseDDP.cpp:178-183, 273-277) and carried in
// ProbState::opt_reb / opt_pen, so an assignment overwrites them with the record's values.  The
// capture (cap_reb / cap_pen) is taken again at the next solve's first AL iteration and is not
// touched here, as `_option = o` touches no local of solve().
//
// List-driven: a lane per changed problem, work proportional to their number, never to the batch.
// No LDS, no atomics; the only indices read from memory are the list's (problem, record) pairs,
// which the host built and checked (problem < B, record < MAXO); every store is a vector store.
//
// In its own translation unit: the neighbours of the solve's kernels stay as they are (the fp32
// build's results are pinned to their code generation).
#include "mhpc_launch.h"

namespace MHPC_NS {

__global__ __launch_bounds__(64) void k_set_options(DevBufs d, int* oid, int n, const int* ent,
                                                    int state) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int b = ent[2 * i], o = ent[2 * i + 1];
  oid[b] = o;
  if (!state) return;
  const OptRec& r = d.opt[o];
  ProbState* st = &d.st[b];
  st->opt_reb = r.ReB_active ? 1 : 0;
  st->opt_pen = r.update_penalty;
}

hipError_t launch_set_options(const DevBufs& d, int* oid, int n, const int* ent, int state,
                              hipStream_t s) {
  if (n < 1) return hipSuccess;
  hipLaunchKernelGGL(k_set_options, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d, oid, n, ent,
                     state);
  return hipGetLastError();
}

}  // namespace MHPC_NS
