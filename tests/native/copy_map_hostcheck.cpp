// Host check of the re-stride map of mhpc_copy_problems (csrc/mhpc_copy_map.h), the code the copy
// kernel runs: one synthetic problem is copied between two sets of host arrays through
// run_of / piece_of / width_of, every source element carrying a unique tag and every destination
// element another, and the result is compared with the copy written out element by element from
// the arrays' index formulas (mhpc_solver.h).  Checked for 8- and 4-byte elements, for the knot
// strides (7,7), (7,12), (12,7) and for stores of differing shape, present on one side only or
// absent:
//  * every element of the problem's knots lands at the destination's index, the tails of K, du, G
//    and the uncovered store rows are zero, and nothing else is written;
//  * every run lies inside both arrays, the blocks of the launch's (run, chunk) table write every
//    byte of it exactly once and none is empty, and width_of divides every offset and length it
//    is used for.
// Exit status 0 and "ok" when all hold; the first violated checks are printed otherwise.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_copy_map.h"

using namespace mhpc_copy;

namespace {
int failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (++failures <= 20) {               \
        printf("FAILED %s: ", #cond);       \
        printf(__VA_ARGS__);                \
        printf("\n");                       \
      }                                     \
    }                                       \
  } while (0)

constexpr int ST_ELEMS = 37, CARRY_ELEMS = 53;  // stand-ins for ProbState / BwsCarry

// elements of each array for a batch of B problems
std::vector<size_t> elems(const Dims& d, int B) {
  std::vector<size_t> n(A_N);
  const size_t b = B, NK = d.NK;
  n[A_TRAJ] = b * d.nslot * NK * 24;
  n[A_PAR] = b * NK * 176;
  n[A_REFPOS] = b * NK;
  n[A_K] = b * NK * 56;
  n[A_DU] = b * NK * 4;
  n[A_G] = b * NK * 14;
  n[A_PX] = b * 16 * 196;
  n[A_X0] = b * 14;
  n[A_ST] = b * ST_ELEMS;
  n[A_CARRY] = b * CARRY_ELEMS;
  n[A_CMD] = b * 2;
  n[A_STORE] = b * d.spmax * d.nbk * 98;
  return n;
}

template <class T>
struct Arrays {
  std::vector<T> a[A_N];
  Arrays(const Dims& d, int B, T side) {
    const std::vector<size_t> n = elems(d, B);
    const int sh = sizeof(T) == 8 ? 40 : 26;
    for (int i = 0; i < A_N; ++i) {
      a[i].resize(n[i]);
      for (size_t j = 0; j < n[i]; ++j) a[i][j] = side | ((T)(i + 1) << sh) | (T)(j + 1);
    }
  }
};

// the copy, element by element, from the arrays' index formulas
template <class T>
void expect_copy(const Arrays<T>& s, Arrays<T>& d, const Dims& sd, const Dims& dd, int bs, int bd) {
  const size_t NKs = sd.NK, NKd = dd.NK, NKc = std::min(NKs, NKd), S = dd.nslot, Bs = bs, Bd = bd;
  for (size_t sl = 0; sl < S; ++sl)
    for (size_t k = 0; k < NKc; ++k)
      for (size_t i = 0; i < 24; ++i)
        d.a[A_TRAJ][((Bd * S + sl) * NKd + k) * 24 + i] = s.a[A_TRAJ][((Bs * S + sl) * NKs + k) * 24 + i];
  for (size_t k = 0; k < NKc; ++k) {
    for (size_t c = 0; c < 18; ++c)
      for (size_t i = 0; i < 9; ++i)
        d.a[A_PAR][Bd * NKd * 176 + (c * NKd + k) * 9 + i] = s.a[A_PAR][Bs * NKs * 176 + (c * NKs + k) * 9 + i];
    for (size_t i = 0; i < 14; ++i)
      d.a[A_PAR][Bd * NKd * 176 + 162 * NKd + k * 14 + i] = s.a[A_PAR][Bs * NKs * 176 + 162 * NKs + k * 14 + i];
    d.a[A_REFPOS][Bd * NKd + k] = s.a[A_REFPOS][Bs * NKs + k];
  }
  const int arr[3] = {A_K, A_DU, A_G};
  const size_t per[3] = {56, 4, 14};
  for (int q = 0; q < 3; ++q)
    for (size_t k = 0; k < NKd; ++k)
      for (size_t i = 0; i < per[q]; ++i)
        d.a[arr[q]][(Bd * NKd + k) * per[q] + i] = k < NKc ? s.a[arr[q]][(Bs * NKs + k) * per[q] + i] : T(0);
  const int rec_arr[5] = {A_PX, A_X0, A_ST, A_CARRY, A_CMD};
  const size_t rec[5] = {16 * 196, 14, ST_ELEMS, CARRY_ELEMS, 2};
  for (int q = 0; q < 5; ++q)
    for (size_t i = 0; i < rec[q]; ++i) d.a[rec_arr[q]][Bd * rec[q] + i] = s.a[rec_arr[q]][Bs * rec[q] + i];
  for (size_t p = 0; p < (size_t)dd.spmax; ++p)
    for (size_t k = 0; k < (size_t)dd.nbk; ++k)
      for (size_t i = 0; i < 98; ++i)
        d.a[A_STORE][((Bd * dd.spmax + p) * dd.nbk + k) * 98 + i] =
            p < (size_t)sd.spmax && k < (size_t)sd.nbk ? s.a[A_STORE][((Bs * sd.spmax + p) * sd.nbk + k) * 98 + i]
                                                       : T(0);
}

template <class T>
void run_case(const char* what, Dims sd, Dims dd, int Bs, int Bd, int bs, int bd, size_t chunk) {
  const T src_side = 0, dst_side = (T)1 << (8 * sizeof(T) - 1);
  const Arrays<T> src(sd, Bs, src_side);
  Arrays<T> want(dd, Bd, dst_side), got(dd, Bd, dst_side);
  expect_copy(src, want, sd, dd, bs, bd);
  const Sizes z = {(int)sizeof(T), (int)(ST_ELEMS * sizeof(T)), (int)(CARRY_ELEMS * sizeof(T))};
  std::vector<unsigned char> hits[A_N];
  for (int i = 0; i < A_N; ++i) hits[i].assign(got.a[i].size() * sizeof(T), 0);
  CHECK(n_runs(dd) == dd.nslot + 19 + 9 + dd.spmax, "%s: run count", what);
  // the launch's blocks: the (run, chunk) table of one pair, each entry one block's work
  std::vector<int> table(block_table(sd, dd, z, chunk, nullptr));
  CHECK(block_table(sd, dd, z, chunk, table.data()) == (int)table.size(), "%s: table size", what);
  for (size_t e = 0; e <= table.size(); ++e) {
    // (one entry past the table: a chunk past a run's end, which must be empty)
    const int r = e < table.size() ? (table[e] & 0xffff) : 0;
    const Run q = run_of(sd, dd, z, bs, bd, r);
    const int c = e < table.size() ? (table[e] >> 16) : chunks_of(q, chunk);
    CHECK(r < n_runs(dd) && c >= 0, "%s: entry %zu names run %d chunk %d", what, e, r, c);
    CHECK(q.arr >= 0 && q.arr < A_N, "%s: run %d array %d", what, r, q.arr);
    if (r >= n_runs(dd) || q.arr < 0 || q.arr >= A_N) continue;
    const size_t sbytes = src.a[q.arr].size() * sizeof(T), dbytes = got.a[q.arr].size() * sizeof(T);
    CHECK(q.ncopy == 0 || q.so + q.ncopy <= sbytes, "%s: run %d reads past the source array", what, r);
    CHECK(q.dof + q.ncopy + q.nzero <= dbytes, "%s: run %d writes past the destination array", what, r);
    if ((q.ncopy && q.so + q.ncopy > sbytes) || q.dof + q.ncopy + q.nzero > dbytes) continue;
    const size_t w = (size_t)width_of(q);
    CHECK(w == 16 || w == 8 || (w == 4 && sizeof(T) == 4), "%s: run %d width %zu", what, r, w);
    CHECK(q.so % w == 0 && q.dof % w == 0, "%s: run %d misaligned for width %zu", what, r, w);
    const char* s = (const char*)src.a[q.arr].data() + q.so;
    char* d = (char*)got.a[q.arr].data() + q.dof;
    const Piece p = piece_of(q, c, chunk);
    CHECK(p.c0 <= p.c1 && p.c1 <= p.z1 && p.z1 <= q.ncopy + q.nzero, "%s: run %d piece %d order", what, r, c);
    CHECK(p.c1 <= q.ncopy || p.c0 == p.c1, "%s: run %d piece %d copies past ncopy", what, r, c);
    CHECK((p.c1 - p.c0) % w == 0 && (p.z1 - p.c1) % w == 0 && p.c0 % w == 0,
          "%s: run %d piece %d not a multiple of the width", what, r, c);
    if (e < table.size()) CHECK(p.c0 < p.z1, "%s: run %d piece %d is an empty block", what, r, c);
    else CHECK(p.c0 == p.z1, "%s: run %d piece past the end is not empty", what, r);
    if (p.c1 > p.c0) memcpy(d + p.c0, s + p.c0, p.c1 - p.c0);
    if (p.z1 > p.c1) memset(d + p.c1, 0, p.z1 - p.c1);
    for (size_t i = p.c0; i < p.z1; ++i) ++hits[q.arr][q.dof + i];
  }
  for (int i = 0; i < A_N; ++i) {
    for (size_t j = 0; j < got.a[i].size(); ++j)
      CHECK(got.a[i][j] == want.a[i][j], "%s: array %d element %zu", what, i, j);
    for (size_t j = 0; j < hits[i].size(); ++j) CHECK(hits[i][j] <= 1, "%s: array %d byte %zu written twice", what, i, j);
  }
}

template <class T>
void all_cases() {
  const int nslot = 4;
  const int nk[3][2] = {{7, 7}, {7, 12}, {12, 7}};  // (12, 7): the source problem has a 7-knot layout
  // (nbk, spmax) of the source / destination store; spmax = 0: none
  const int st[6][4] = {{9, 5, 9, 5}, {9, 5, 11, 4}, {11, 4, 7, 6}, {0, 0, 9, 5}, {9, 5, 0, 0}, {0, 0, 0, 0}};
  char what[96];
  for (const auto& k : nk)
    for (const auto& s : st)
      for (size_t chunk : {(size_t)48, (size_t)16384}) {
        snprintf(what, sizeof what, "%zu-byte NK %d->%d store (%d,%d)->(%d,%d) chunk %zu", sizeof(T), k[0],
                 k[1], s[0], s[1], s[2], s[3], chunk);
        run_case<T>(what, Dims{k[0], nslot, s[0], s[1]}, Dims{k[1], nslot, s[2], s[3]}, 3, 2, 2, 1, chunk);
        run_case<T>(what, Dims{k[0], nslot, s[0], s[1]}, Dims{k[1], nslot, s[2], s[3]}, 2, 3, 0, 2, chunk);
      }
  // inside one handle: the same dimensions on both sides, another problem of the same arrays
  run_case<T>("same dimensions", Dims{12, nslot, 9, 5}, Dims{12, nslot, 9, 5}, 3, 3, 1, 2, 16384);
}
}  // namespace

int main() {
  all_cases<uint64_t>();
  all_cases<uint32_t>();
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
