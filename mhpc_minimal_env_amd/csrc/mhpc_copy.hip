// Device code of mhpc_copy_problems: destination problem pairs[2i + 1] of one handle becomes a
// copy of source problem pairs[2i] of another (or of the same) handle, with every packed array
// re-strided from the source's knot stride and store shape to the destination's.
//
// Pure memory traffic, list-driven: one launch, a block per (pair, run, chunk) where the runs are
// the contiguous pieces of a problem that mhpc_copy_map.h enumerates and a chunk is COPY_CH bytes
// of a run (the (run, chunk) table of one pair is built on the host: no empty blocks).  Device
// work is proportional to the number of pairs, never to either batch.  A block serves one pair
// and one run, so both problem numbers, both strides and with them both offsets and the access
// width are block-uniform: the pair and the table entry are read through the constant address
// space (scalar loads, as the group table is) and the map is scalar arithmetic.  The lanes stride over
// the chunk's contiguous bytes, each access as wide as width_of proves aligned on both sides, so a
// wave reads and writes whole lines.  No atomics, no LDS, no index taken from array contents (a
// non-finite source copies as bits); every store is a vector store.
//
// In its own translation unit: the neighbours of the solve's kernels stay as they are (the fp32
// build's results are pinned to their code generation).
#include "mhpc_copy_map.h"
#include "mhpc_launch.h"

namespace MHPC_NS {

static_assert(mhpc_copy::KS == KS && mhpc_copy::PS == PS && mhpc_copy::PS_JAC == PS_JAC &&
                  mhpc_copy::MAXP == MAXP && mhpc_copy::SREC == kStoreRec,
              "mhpc_copy_map.h restates the record widths of mhpc_solver.h / mhpc_launch.h");
static_assert(sizeof(ProbState) % 8 == 0 && sizeof(BwsCarry) % 8 == 0 && sizeof(Cmd) == 2 * sizeof(real),
              "whole-record runs");

constexpr size_t COPY_CH = 16384;  // bytes of a run a block moves: 4 passes of 256 lanes x 16 B

struct CopyArgs {
  const char* src[mhpc_copy::A_N];
  char* dst[mhpc_copy::A_N];
  mhpc_copy::Dims sd, dd;
  const int* pairs;   // [n][2]: source problem, destination problem
  const int* blocks;  // [gridDim.y]: run | chunk << 16 of each block of a pair (block_table)
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) int CInt;

template <class V>
static __device__ __forceinline__ void copy_piece(const char* s, char* d, const mhpc_copy::Piece& p) {
  const size_t t = (size_t)threadIdx.x * sizeof(V), step = 256 * sizeof(V);
  for (size_t i = p.c0 + t; i < p.c1; i += step) *(V*)(d + i) = *(const V*)(s + i);
  const V zero = {};
  for (size_t i = p.c1 + t; i < p.z1; i += step) *(V*)(d + i) = zero;
}

__global__ __launch_bounds__(256) void k_copy_problems(CopyArgs a) {
  using namespace mhpc_copy;
  const int bs = ((CInt*)a.pairs)[2 * blockIdx.x], bd = ((CInt*)a.pairs)[2 * blockIdx.x + 1];
  const Sizes z = {(int)sizeof(real), (int)sizeof(ProbState), (int)sizeof(BwsCarry)};
  const int rc = ((CInt*)a.blocks)[blockIdx.y];
  const Run r = run_of(a.sd, a.dd, z, bs, bd, rc & 0xffff);
  const Piece p = piece_of(r, rc >> 16, COPY_CH);
  if (p.c0 >= p.z1) return;
  const char* s = a.src[r.arr] + r.so;
  char* d = a.dst[r.arr] + r.dof;
  const int w = width_of(r);
  if (w == 16)
    copy_piece<u32x4>(s, d, p);
  else if (w == 8)
    copy_piece<u32x2>(s, d, p);
  else
    copy_piece<unsigned int>(s, d, p);
}

static mhpc_copy::Dims dims_of(const CopySide& c) {
  return mhpc_copy::Dims{c.NK, c.nslot, c.store ? c.nbk : 0, c.store ? c.spmax : 0};
}
static void bases_of(const CopySide& c, const char** p) {
  using namespace mhpc_copy;
  p[A_TRAJ] = (const char*)c.d.traj;
  p[A_PAR] = (const char*)c.d.par;
  p[A_REFPOS] = (const char*)c.d.refpos;
  p[A_K] = (const char*)c.d.K;
  p[A_DU] = (const char*)c.d.du;
  p[A_G] = (const char*)c.d.G;
  p[A_PX] = (const char*)c.d.px;
  p[A_X0] = (const char*)c.d.x0;
  p[A_ST] = (const char*)c.d.st;
  p[A_CARRY] = (const char*)c.d.carry;
  p[A_CMD] = (const char*)c.d.cmd;
  p[A_STORE] = (const char*)c.store;
}

int copy_block_table(const CopySide& src, const CopySide& dst, int* out) {
  const mhpc_copy::Sizes z = {(int)sizeof(real), (int)sizeof(ProbState), (int)sizeof(BwsCarry)};
  return mhpc_copy::block_table(dims_of(src), dims_of(dst), z, COPY_CH, out);
}

hipError_t launch_copy_problems(const CopySide& src, const CopySide& dst, int n, const int* pairs,
                                int nblk, const int* blocks, hipStream_t s) {
  using namespace mhpc_copy;
  CopyArgs a;
  const char* db[A_N];
  bases_of(src, a.src);
  bases_of(dst, db);
  for (int i = 0; i < A_N; ++i) a.dst[i] = const_cast<char*>(db[i]);
  a.sd = dims_of(src);
  a.dd = dims_of(dst);
  a.pairs = pairs;
  a.blocks = blocks;
  hipLaunchKernelGGL(k_copy_problems, dim3((unsigned)n, (unsigned)nblk), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace MHPC_NS
