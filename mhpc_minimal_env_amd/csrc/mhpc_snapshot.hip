// Device path of mhpc_snapshot_problems / mhpc_restore_problems: the staging side of a round and
// the copies between it and the blob's payload.
//
// A round's staging buffer is a CopySide like a handle's (mhpc_snapshot_map.h: R problems, knot
// stride = the longest listed layout, the source's slot count and store shape, every array's base
// aligned), so pack and unpack are launch_copy_problems itself -- k_copy_problems with the staging
// side as its destination or its source.  That keeps the copy kernel's properties for both
// directions (block-uniform pair and run read through the constant address space, the widest
// access both sides' alignment proves, whole-line vector stores, no atomics, no index from array
// contents) and leaves one re-stride map for the copy, the snapshot and their host checks.  Pack
// writes every byte of the staging records it covers (the staging stride never exceeds the
// source's, and run_of zero-fills a store buffer's tail), so no byte of a blob comes from
// uninitialised memory.
//
// In its own translation unit, as mhpc_copy.hip is: the solve's kernels keep their neighbours.
#include "mhpc_launch.h"
#include "mhpc_snapshot_map.h"

namespace MHPC_NS {

static_assert(mhpc_copy::A_N == 12, "snap_side names every array of the map");

static mhpc_copy::Sizes snap_sizes() {
  return mhpc_copy::Sizes{(int)sizeof(real), (int)sizeof(ProbState), (int)sizeof(BwsCarry)};
}

CopySide snap_side(void* staging, int R, int NK, int nslot, int nbk, int spmax) {
  using namespace mhpc_copy;
  const Dims d{NK, nslot, nbk, spmax};
  const Sizes z = snap_sizes();
  char* b = (char*)staging;
  auto at = [&](int a) { return b + mhpc_snap::stage_off(d, z, a, (size_t)R); };
  CopySide c{};
  c.d.traj = (real*)at(A_TRAJ);
  c.d.par = (real*)at(A_PAR);
  c.d.refpos = (real*)at(A_REFPOS);
  c.d.K = (real*)at(A_K);
  c.d.du = (real*)at(A_DU);
  c.d.G = (real*)at(A_G);
  c.d.px = (real*)at(A_PX);
  c.d.x0 = (real*)at(A_X0);
  c.d.st = (ProbState*)at(A_ST);
  c.d.carry = (BwsCarry*)at(A_CARRY);
  c.d.cmd = (const Cmd*)at(A_CMD);
  c.store = spmax > 0 ? (real*)at(A_STORE) : nullptr;
  c.NK = NK;
  c.nslot = nslot;
  c.nbk = nbk;
  c.spmax = spmax;
  return c;
}

size_t snap_stage_bytes(int R, int NK, int nslot, int nbk, int spmax) {
  return mhpc_snap::stage_bytes(mhpc_copy::Dims{NK, nslot, nbk, spmax}, snap_sizes(), (size_t)R);
}

// `count` consecutive entries from `entry` on between a blob's payload (of n entries) and the
// staging records from `slot` on: one asynchronous copy per array, queued on s.
hipError_t snap_move(void* staging, int R, int NK, int nslot, int nbk, int spmax, char* payload,
                     int n, int entry, int slot, int count, bool to_host, hipStream_t s) {
  using namespace mhpc_copy;
  const Dims d{NK, nslot, nbk, spmax};
  const Sizes z = snap_sizes();
  for (int a = 0; a < A_N; ++a) {
    const size_t rec = mhpc_snap::rec_bytes(d, z, a);
    if (rec == 0) continue;
    char* dev = (char*)staging + mhpc_snap::stage_off(d, z, a, (size_t)R) + (size_t)slot * rec;
    char* host = payload + mhpc_snap::payload_off(d, z, a, (size_t)n) + (size_t)entry * rec;
    const hipError_t e = to_host ? hipMemcpyAsync(host, dev, (size_t)count * rec, hipMemcpyDeviceToHost, s)
                                 : hipMemcpyAsync(dev, host, (size_t)count * rec, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace MHPC_NS
