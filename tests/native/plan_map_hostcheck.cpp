// Host check of the window map of mhpc_export_plan_device (csrc/mhpc_plan_map.h), the header
// k_plan_export and the runtime's validation run, compiled by plain g++
// (tests/test_plan_map_host.py, also under the address and undefined-behaviour sanitizers).
// Synthetic layouts: C3-like (80, 80 whole-body + 2 SRB phases), SRB-only, one whole-body phase, a
// layout whose ko is not the running sum of N (rotated buffers), a phase with N = 2.  Windows, each
// for rows of r = 14 and r = 6 (r = 6 only where the layout's state size is 6): W = 1 at the first
// and the last step, a window starting 3 steps before every phase boundary with W = 5, a window
// reaching past the last step, W = all steps.  For each window and each output kind:
//   * every element of the [W][c] block is classified exactly once (its (w, c) is its own, and
//     the block's elements are all visited);
//   * an element is a zero exactly when its row is past `valid` or its column past the state size;
//   * every other element's source offset is the one mhpc_ctrl::nom_off / gain_off / du_off (and
//     the G row) name for knot_of(first + w), lies inside its array (each is read, so an offset
//     outside is a sanitizer report) and is named by no other element of the block;
//   * no row names a phase's last knot;
//   * valid = min(W, n_steps - first).
#include <cstdio>
#include <set>
#include <vector>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_plan_map.h"

namespace mc = mhpc_ctrl;
namespace pm = mhpc_plan_map;

struct Lay {
  const char* name;
  int P, n_wb;
  std::vector<int> N, ko;
};

static int fails = 0;
static long checked = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++fails;                                 \
    }                                          \
  } while (0)

static void check_window(const Lay& L, int r, int first, int W) {
  const pm::Lay ml = {L.P, L.n_wb, L.N.data(), L.ko.data()};
  const int n = mc::state_size(L.n_wb), ns = mc::n_steps(L.P, L.n_wb, L.N.data());
  int NK = 0;
  for (int p = 0; p < L.P; ++p) NK = L.ko[p] + L.N[p] > NK ? L.ko[p] + L.N[p] : NK;
  NK += 3;  // a handle's knot stride may exceed the layout's knots
  const int B = 3, nslot = 4, b = 2, slot = 1;
  const pm::Dims D = {NK, nslot};
  const std::vector<double> traj((size_t)B * nslot * NK * mc::KS, 1.0), K((size_t)B * NK * mc::KW, 1.0),
      du((size_t)B * NK * mc::UW, 1.0), G((size_t)B * NK * pm::GW, 1.0);
  const std::vector<int> mode(L.P, 1);

  const int nv = pm::valid(ns, first, W);
  const int want_nv = ns - first < W ? ns - first : W;
  CHECK(nv == want_nv && nv >= 1 && nv <= W, "%s r%d first %d W %d: valid %d, want %d", L.name, r, first, W, nv, want_nv);

  for (int kind = 0; kind < pm::NKIND; ++kind) {
    const int nc = pm::cols(kind, r);
    const int want_nc = kind == pm::X_NOM || kind == pm::VX ? r : kind == pm::GAIN ? 4 * r : kind == pm::MODE ? 1 : 4;
    CHECK(nc == want_nc, "cols of kind %d", kind);
    const long blk = pm::block(kind, r, W);
    CHECK(blk == (long)W * nc, "block of kind %d", kind);
    std::vector<int> hits((size_t)blk, 0);
    std::set<size_t> srcs;
    double sum = 0;
    long nonzero = 0;
    for (long e = 0; e < blk; ++e) {
      const pm::Elem q = pm::elem(kind, r, ml, D, b, slot, first, nv, e);
      ++checked;
      CHECK(q.w >= 0 && q.w < W && q.c >= 0 && q.c < nc && (long)q.w * nc + q.c == e,
            "%s kind %d: element %ld -> (%d, %d)", L.name, kind, e, q.w, q.c);
      if (q.w < 0 || q.w >= W || q.c < 0 || q.c >= nc) continue;
      ++hits[(size_t)q.w * nc + q.c];
      const int col = kind == pm::GAIN ? q.c % r : q.c;
      const bool padded = (kind == pm::X_NOM || kind == pm::VX || kind == pm::GAIN) && col >= n;
      CHECK(q.zero == (q.w >= nv || padded), "%s kind %d: element %ld zero %d (row %d of %d valid, column %d of %d)",
            L.name, kind, e, (int)q.zero, q.w, nv, col, n);
      if (q.zero) continue;
      ++nonzero;
      mc::Knot k{-1, -1, -1};
      const bool ok = mc::knot_of(L.P, L.n_wb, L.N.data(), L.ko.data(), first + q.w, &k);
      CHECK(ok, "%s: step %d of a valid row refused", L.name, first + q.w);
      if (!ok) continue;
      // never a phase's last knot, across a boundary or not
      CHECK(k.k < L.N[k.phase] - 1 && k.kk != L.ko[k.phase] + L.N[k.phase] - 1, "%s: step %d names a last knot",
            L.name, first + q.w);
      CHECK(q.phase == k.phase, "%s kind %d: element %ld phase", L.name, kind, e);
      size_t want = 0, size = 0;
      const double* arr = nullptr;
      switch (kind) {
        case pm::X_NOM: want = mc::nom_off(NK, nslot, b, slot, k.kk) + q.c, size = traj.size(), arr = traj.data(); break;
        case pm::U_NOM: want = mc::nom_off(NK, nslot, b, slot, k.kk) + n + q.c, size = traj.size(), arr = traj.data(); break;
        case pm::Y: want = mc::nom_off(NK, nslot, b, slot, k.kk) + n + 4 + q.c, size = traj.size(), arr = traj.data(); break;
        case pm::GAIN: want = mc::gain_off(NK, b, k.kk) + (size_t)(q.c / r) * n + col, size = K.size(), arr = K.data(); break;
        case pm::DU: want = mc::du_off(NK, b, k.kk) + q.c, size = du.size(), arr = du.data(); break;
        case pm::VX: want = ((size_t)b * NK + k.kk) * 14 + q.c, size = G.size(), arr = G.data(); break;
        default: want = (size_t)k.phase, size = mode.size(); break;
      }
      CHECK(q.src == want, "%s kind %d: element %ld source %zu, want %zu", L.name, kind, e, q.src, want);
      CHECK(q.src < size, "%s kind %d: element %ld source %zu outside %zu", L.name, kind, e, q.src, size);
      if (q.src >= size) continue;
      sum += arr ? arr[q.src] : (double)mode[q.src];
      if (kind != pm::MODE)
        CHECK(srcs.insert(q.src).second, "%s kind %d: element %ld repeats a source", L.name, kind, e);
      // inside the knot's own record: x, u, y within the 24, the gain within the 4 n dense words
      if (kind == pm::X_NOM || kind == pm::U_NOM || kind == pm::Y)
        CHECK(q.src - mc::nom_off(NK, nslot, b, slot, k.kk) < (size_t)mc::KS, "%s kind %d: outside the record", L.name, kind);
      if (kind == pm::GAIN)
        CHECK(q.src - mc::gain_off(NK, b, k.kk) < (size_t)(4 * n), "%s: gain outside the dense words", L.name);
    }
    for (long e = 0; e < blk; ++e) CHECK(hits[(size_t)e] == 1, "%s kind %d: element %ld classified %d times", L.name, kind, e, hits[(size_t)e]);
    const int live = kind == pm::X_NOM || kind == pm::VX ? (n < r ? n : r) : kind == pm::GAIN ? 4 * (n < r ? n : r) : nc;
    CHECK(nonzero == (long)nv * live && sum == (double)nonzero, "%s kind %d: %ld sources for %d rows of %d", L.name, kind,
          nonzero, nv, live);
  }
}

static void check_layout(const Lay& L) {
  const int nph = mc::n_phases(L.P, L.n_wb), n = mc::state_size(L.n_wb);
  const int ns = mc::n_steps(L.P, L.n_wb, L.N.data());
  for (int r : {14, 6}) {
    if (r < n) continue;  // rows of 6 belong to handles whose problems are all SRB-only
    check_window(L, r, 0, 1);
    check_window(L, r, ns - 1, 1);
    int off = 0;
    for (int p = 0; p < nph; ++p) {  // 3 steps before the end of each phase, W = 5
      off += L.N[p] - 1;
      if (off - 3 >= 0) check_window(L, r, off - 3, 5);
    }
    check_window(L, r, ns > 2 ? ns - 2 : 0, 6);  // past the last step
    check_window(L, r, 0, ns);                   // all steps
    check_window(L, r, 0, ns + 7);
  }
}

int main() {
  const std::vector<Lay> lays = {
      {"c3", 4, 2, {80, 80, 50, 50}, {0, 80, 160, 210}},
      {"srb-only", 3, 0, {50, 30, 2}, {0, 50, 80}},
      {"one-wb", 1, 1, {120}, {0}},
      {"rotated", 4, 2, {80, 100, 50, 50}, {100, 0, 230, 180}},
      {"n2", 3, 2, {2, 5, 9}, {0, 2, 7}},
      {"n2-only", 2, 1, {2, 40}, {0, 2}},
  };
  for (const Lay& L : lays) check_layout(L);
  {  // the stated numbers: C3, first 76, W 5 is steps 76..80 = knots 76, 77, 78 of phase 0, then
     // knots 0, 1 of phase 1 at kk 80, 81 -- never kk 79, phase 0's last knot
    const Lay& L = lays[0];
    const pm::Lay ml = {L.P, L.n_wb, L.N.data(), L.ko.data()};
    const pm::Dims D = {260, 3};
    const int kk_want[5] = {76, 77, 78, 80, 81};
    CHECK(pm::valid(158, 76, 5) == 5 && pm::valid(158, 156, 6) == 2 && pm::valid(158, 0, 158) == 158 &&
              pm::valid(49, 0, 158) == 49,
          "c3: valid");
    for (int w = 0; w < 5; ++w) {
      const pm::Elem q = pm::elem(pm::DU, 14, ml, D, 0, 0, 76, 5, (long)w * 4);
      CHECK(!q.zero && q.src == (size_t)kk_want[w] * 4 && q.phase == (w < 3 ? 0 : 1), "c3: window row %d at kk %zu", w,
            q.src / 4);
    }
    // the rotated layout: step 79 is phase 1 at kk 0
    const Lay& R = lays[3];
    const pm::Lay mr = {R.P, R.n_wb, R.N.data(), R.ko.data()};
    const pm::Elem q = pm::elem(pm::VX, 14, mr, D, 1, 0, 77, 4, 2 * 14 + 3);
    CHECK(!q.zero && q.phase == 1 && q.src == ((size_t)1 * 260 + 0) * 14 + 3, "rotated: step 79");
    // an SRB-only problem in rows of 14: K's row i starts at i * 6 of the dense words
    const Lay& S = lays[1];
    const pm::Lay ms = {S.P, S.n_wb, S.N.data(), S.ko.data()};
    const pm::Elem g = pm::elem(pm::GAIN, 14, ms, D, 0, 0, 0, 1, 2 * 14 + 5);
    CHECK(!g.zero && g.src == 2 * 6 + 5, "srb-only: gain row 2 column 5");
    CHECK(pm::elem(pm::GAIN, 14, ms, D, 0, 0, 0, 1, 2 * 14 + 6).zero, "srb-only: gain column 6 is a zero");
  }
  if (fails) {
    std::printf("%d failure(s)\n", fails);
    return 1;
  }
  std::printf("plan_map_hostcheck: %zu layouts, %ld elements ok\n", lays.size(), checked);
  return 0;
}
