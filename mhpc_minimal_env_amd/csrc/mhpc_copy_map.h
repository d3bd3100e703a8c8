// The re-stride map of mhpc_copy_problems: where each piece of one problem's device state lies in
// the source handle's arrays and where it goes in the destination's.  Two handles differ in their
// knot stride NK (the largest knot count of each handle's layouts) and in the shape of their
// phase-buffer store (nbk knots a buffer, spmax buffers a problem), so a problem is not one
// contiguous block: it is a fixed list of contiguous runs, each with its own source and
// destination offset, cut into chunks for the launch (block_table).  The kernel (mhpc_copy.hip)
// and the host check (tests/native/copy_map_hostcheck.cpp) walk the same list with the same code;
// everything here is plain arithmetic on the handles' dimensions, no index comes from array
// contents.
//
// Runs of one (source problem bs, destination problem bd) pair, in bytes from each array's base:
//   traj    nslot runs   slot s: knots [0, NKc) of [b][s][NK][KS]           NKc = min(NK_s, NK_d)
//   par     19 runs      column block c < 18: [NKc][9] at (b NK PS + c NK 9); then the cost
//                        derivatives [NKc][14] at (b NK PS + PS_JAC NK)     (par_col / par_jac)
//   refpos, K, du, G     knots [0, NKc) of [b][NK][1 | 56 | 4 | 14]; K, du, G: the rest of the
//                        destination's stride is zeroed (what k_reset_list leaves there)
//   px, x0, st, carry, cmd   the problem's whole record
//   store   spmax_d runs buffer p: knots [0, min(nbk_s, nbk_d)) of [b][spmax][nbk][SREC] when the
//                        source has buffer p, the rest of the destination's buffer zeroed
// The tail knots [NKc, NK_d) of traj, par and refpos stay as they are, as after a reset.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MHPC_COPY_HD __host__ __device__
#else
#define MHPC_COPY_HD
#endif

namespace mhpc_copy {

// record widths of mhpc_solver.h / mhpc_launch.h (mhpc_copy.hip asserts that they agree)
constexpr int KS = 24, PS = 176, PS_JAC = 162, NCOL = 18, MAXP = 16, SREC = KS + 56 + 4 + 14;

enum Arr { A_TRAJ = 0, A_PAR, A_REFPOS, A_K, A_DU, A_G, A_PX, A_X0, A_ST, A_CARRY, A_CMD, A_STORE, A_N };

struct Dims {
  int NK, nslot;    // knot stride, trajectory slots (nslot is handle-wide and equal on both sides)
  int nbk, spmax;   // phase-buffer store: knots a buffer, buffers a problem (spmax = 0: no store)
};
struct Sizes {
  int real, st, carry;  // bytes of the arithmetic type, of ProbState and of BwsCarry
};
struct Run {
  int arr;
  size_t so, dof;        // byte offsets from the source / destination array's base
  size_t ncopy, nzero;   // bytes copied, then bytes zeroed right after them in the destination
};

MHPC_COPY_HD inline int n_runs(const Dims& d) { return d.nslot + (NCOL + 1) + 9 + d.spmax; }

MHPC_COPY_HD inline Run run_of(const Dims& s, const Dims& d, const Sizes& z, int bs, int bd, int r) {
  const size_t E = (size_t)z.real, Bs = (size_t)bs, Bd = (size_t)bd;
  const size_t NKs = (size_t)s.NK, NKd = (size_t)d.NK, NKc = NKs < NKd ? NKs : NKd;
  Run o;
  o.nzero = 0;
  if (r < d.nslot) {
    o.arr = A_TRAJ;
    o.so = (Bs * d.nslot + r) * NKs * KS * E;
    o.dof = (Bd * d.nslot + r) * NKd * KS * E;
    o.ncopy = NKc * KS * E;
    return o;
  }
  r -= d.nslot;
  if (r <= NCOL) {
    o.arr = A_PAR;
    const size_t in_s = r < NCOL ? (size_t)r * NKs * 9 : (size_t)PS_JAC * NKs;
    const size_t in_d = r < NCOL ? (size_t)r * NKd * 9 : (size_t)PS_JAC * NKd;
    o.so = (Bs * NKs * PS + in_s) * E;
    o.dof = (Bd * NKd * PS + in_d) * E;
    o.ncopy = NKc * (r < NCOL ? 9 : 14) * E;
    return o;
  }
  r -= NCOL + 1;
  if (r < 4) {  // refpos, K, du, G: [b][NK][per]
    const int per = r == 0 ? 1 : r == 1 ? 56 : r == 2 ? 4 : 14;
    o.arr = A_REFPOS + r;
    o.so = Bs * NKs * per * E;
    o.dof = Bd * NKd * per * E;
    o.ncopy = NKc * per * E;
    if (r > 0) o.nzero = (NKd - NKc) * per * E;
    return o;
  }
  if (r < 9) {  // one record a problem
    const size_t rec = r == 4 ? (size_t)MAXP * 196 * E : r == 5 ? 14 * E : r == 6 ? (size_t)z.st
                     : r == 7 ? (size_t)z.carry : 2 * E;
    o.arr = A_PX + (r - 4);
    o.so = Bs * rec;
    o.dof = Bd * rec;
    o.ncopy = rec;
    return o;
  }
  r -= 9;  // store buffer r of the destination
  const size_t nbs = (size_t)s.nbk, nbd = (size_t)d.nbk;
  o.arr = A_STORE;
  o.so = (Bs * s.spmax + r) * nbs * SREC * E;
  o.dof = (Bd * d.spmax + r) * nbd * SREC * E;
  o.ncopy = r < s.spmax ? (nbs < nbd ? nbs : nbd) * SREC * E : 0;
  o.nzero = nbd * SREC * E - o.ncopy;
  return o;
}

// Widest access (16, 8 or 4 bytes) that both offsets and both lengths of a run are multiples of:
// every access of the run is then aligned on both sides (the arrays' bases are allocations).
MHPC_COPY_HD inline int width_of(const Run& r) {
  const size_t a = r.so | r.dof | r.ncopy | r.nzero;
  return a % 16 == 0 ? 16 : a % 8 == 0 ? 8 : 4;
}

// Chunk c of a run (chunk bytes of it, a multiple of 16): copy [c0, c1), zero [c1, z1), as
// offsets into the run.  An empty piece has c0 == z1.
struct Piece {
  size_t c0, c1, z1;
};
MHPC_COPY_HD inline Piece piece_of(const Run& r, int c, size_t chunk) {
  const size_t end = r.ncopy + r.nzero, a = (size_t)c * chunk;
  Piece p;
  p.c0 = a < end ? a : end;
  p.z1 = a + chunk < end ? a + chunk : end;
  p.c1 = p.c0 > r.ncopy ? p.c0 : (p.z1 < r.ncopy ? p.z1 : r.ncopy);
  return p;
}
MHPC_COPY_HD inline int chunks_of(const Run& r, size_t chunk) {
  return (int)((r.ncopy + r.nzero + chunk - 1) / chunk);
}

// The blocks of one pair: every (run, chunk) with bytes in it, as run | chunk << 16, written to
// out when it is not null; returns their number.  A run's length does not depend on the pair, so
// one table serves the whole list and a launch has no empty block.
inline int block_table(const Dims& s, const Dims& d, const Sizes& z, size_t chunk, int* out) {
  int n = 0;
  for (int r = 0; r < n_runs(d); ++r) {
    const int nc = chunks_of(run_of(s, d, z, 0, 0, r), chunk);
    for (int c = 0; c < nc; ++c, ++n)
      if (out) out[n] = r | c << 16;
  }
  return n;
}

}  // namespace mhpc_copy
