// Host check of the window map of mhpc_import_plan_device (csrc/mhpc_import_map.h), the header
// k_plan_import and the runtime's validation run, compiled by plain g++
// (tests/test_import_map_host.py, also under the address and undefined-behaviour sanitizers).
// Synthetic layouts: C3-like (80, 80 whole-body + 2 SRB phases), SRB-only, one whole-body phase, a
// layout whose ko is not the running sum of N (rotated buffers), a phase with N = 2.  Both scopes;
// windows, each for rows of r = 14 and r = 6 (r = 6 only where the layout's largest state size is
// 6): W = 1 at the first and the last step, a window starting 3 steps before every phase boundary
// with W = 5, a window reaching past the last step, W = all steps and more.  For each window and
// each kind (x_nom, u_nom, K, and the zero gains of an import without K):
//   * every element of the [W][c] block is classified exactly once;
//   * an element is skipped exactly when its row is past `valid` or its column past the state
//     size of the step's own phase (6 in an SRB phase of a whole-body problem under STEPS_ALL);
//   * every other element's destination is the one mhpc_ctrl::nom_off / gain_off name for the
//     scope's knot of step first + w, lies inside its array (each is written, so an offset outside
//     is a sanitizer report), inside the record's own field (x: 0..n, u: n..n+4, never y or the
//     tail; K: the 4 n dense words; zero gains: the 56) and is named by no other element;
//   * no row names a phase's last knot, across a boundary or not;
//   * valid = min(W, n_steps - first), and n_steps of STEPS_ALL counts every phase;
//   * under STEPS_CONTROL every element agrees with mhpc_plan_map.h: skipped where the export
//     stores +0, the destination equal to the export's source.
#include <cstdio>
#include <set>
#include <vector>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_import_map.h"
#include "../../mhpc_minimal_env_amd/csrc/mhpc_plan_map.h"

namespace mc = mhpc_ctrl;
namespace im = mhpc_import_map;
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

// The scope's step map restated: phase and knot of step j, by a plain walk over the phases.
static bool step_ref(const Lay& L, int scope, int j, int* phase, int* k) {
  const int nph = scope == im::STEPS_ALL ? L.P : (L.n_wb > 0 ? L.n_wb : L.P);
  int off = 0;
  for (int p = 0; p < nph; ++p) {
    if (j >= off && j < off + L.N[p] - 1) {
      *phase = p;
      *k = j - off;
      return j >= 0;
    }
    off += L.N[p] - 1;
  }
  return false;
}
static int steps_ref(const Lay& L, int scope) {
  const int nph = scope == im::STEPS_ALL ? L.P : (L.n_wb > 0 ? L.n_wb : L.P);
  int n = 0;
  for (int p = 0; p < nph; ++p) n += L.N[p] - 1;
  return n;
}

static void check_window(const Lay& L, int scope, int r, int first, int W) {
  const im::Lay ml = {L.P, L.n_wb, L.N.data(), L.ko.data()};
  const pm::Lay pl = {L.P, L.n_wb, L.N.data(), L.ko.data()};
  const int ns = im::n_steps(scope, L.P, L.n_wb, L.N.data());
  CHECK(ns == steps_ref(L, scope), "%s scope %d: %d steps", L.name, scope, ns);
  int NK = 0;
  for (int p = 0; p < L.P; ++p) NK = L.ko[p] + L.N[p] > NK ? L.ko[p] + L.N[p] : NK;
  NK += 3;  // a handle's knot stride may exceed the layout's knots
  const int B = 3, nslot = 4, b = 2, slot = 1;
  const im::Dims D = {NK, nslot};
  const pm::Dims PD = {NK, nslot};
  std::vector<double> traj((size_t)B * nslot * NK * mc::KS, 0.0), K((size_t)B * NK * mc::KW, 0.0);

  const int nv = im::valid(ns, first, W);
  const int want_nv = ns - first < W ? ns - first : W;
  CHECK(nv == want_nv && nv >= 1 && nv <= W, "%s r%d first %d W %d: valid %d, want %d", L.name, r, first, W, nv, want_nv);

  std::set<size_t> traj_dst;  // x_nom and u_nom share the record: no element of either twice
  for (int kind = 0; kind < im::NKIND; ++kind) {
    const int nc = im::cols(kind, r);
    const int want_nc = kind == im::X_NOM ? r : kind == im::GAIN ? 4 * r : kind == im::ZGAIN ? 56 : 4;
    CHECK(nc == want_nc, "cols of kind %d", kind);
    const long blk = im::block(kind, r, W);
    CHECK(blk == (long)W * nc, "block of kind %d", kind);
    std::vector<int> hits((size_t)blk, 0);
    std::set<size_t> gain_dst;
    long live = 0, want_live = 0;
    for (long e = 0; e < blk; ++e) {
      const im::Elem q = im::elem(scope, kind, r, ml, D, b, slot, first, nv, e);
      ++checked;
      CHECK(q.w >= 0 && q.w < W && q.c >= 0 && q.c < nc && (long)q.w * nc + q.c == e,
            "%s kind %d: element %ld -> (%d, %d)", L.name, kind, e, q.w, q.c);
      if (q.w < 0 || q.w >= W || q.c < 0 || q.c >= nc) continue;
      ++hits[(size_t)q.w * nc + q.c];
      int ph = -1, k = -1;
      const bool exists = q.w < nv && step_ref(L, scope, first + q.w, &ph, &k);
      CHECK(exists == (q.w < nv), "%s scope %d: step %d of a valid row refused", L.name, scope, first + q.w);
      const int n = exists ? (ph < L.n_wb ? 14 : 6) : 0;
      const int col = kind == im::GAIN ? q.c % r : q.c;
      const bool padded = (kind == im::X_NOM || kind == im::GAIN) && col >= n;
      CHECK(q.skip == (!exists || padded), "%s scope %d kind %d: element %ld skip %d (row %d of %d valid, column %d of %d)",
            L.name, scope, kind, e, (int)q.skip, q.w, nv, col, n);
      if (scope == im::STEPS_CONTROL && kind != im::ZGAIN) {  // the export's map, element for element
        const int pk = kind == im::X_NOM ? pm::X_NOM : kind == im::U_NOM ? pm::U_NOM : pm::GAIN;
        const pm::Elem x = pm::elem(pk, r, pl, PD, b, slot, first, nv, e);
        CHECK(x.zero == q.skip && x.w == q.w && x.c == q.c && (x.zero || (x.src == q.dst && x.phase == q.phase)),
              "%s kind %d: element %ld differs from the export's map", L.name, kind, e);
      }
      if (!exists) continue;
      want_live += padded ? 0 : 1;
      if (q.skip) continue;
      ++live;
      CHECK(k < L.N[ph] - 1, "%s: step %d names a last knot", L.name, first + q.w);
      CHECK(q.phase == ph, "%s kind %d: element %ld phase %d, want %d", L.name, kind, e, q.phase, ph);
      const int kk = L.ko[ph] + k;
      CHECK(kk != L.ko[ph] + L.N[ph] - 1, "%s: step %d names a last knot", L.name, first + q.w);
      const size_t rec = mc::nom_off(NK, nslot, b, slot, kk), gain = mc::gain_off(NK, b, kk);
      size_t want = 0;
      switch (kind) {
        case im::X_NOM: want = rec + q.c; break;
        case im::U_NOM: want = rec + n + q.c; break;
        case im::GAIN: want = gain + (size_t)(q.c / r) * n + col; break;
        default: want = gain + q.c; break;
      }
      CHECK(q.dst == want, "%s kind %d: element %ld destination %zu, want %zu", L.name, kind, e, q.dst, want);
      const bool in_traj = kind == im::X_NOM || kind == im::U_NOM;
      const size_t size = in_traj ? traj.size() : K.size();
      CHECK(q.dst < size, "%s kind %d: element %ld destination %zu outside %zu", L.name, kind, e, q.dst, size);
      if (q.dst >= size) continue;
      (in_traj ? traj : K)[q.dst] += 1.0;  // written: an offset outside is a sanitizer report
      // the record's own field: x in 0..n, u in n..n+4 (never y at n+4..n+8, never the tail)
      if (kind == im::X_NOM) CHECK(q.dst - rec < (size_t)n, "%s: x_nom outside 0..n", L.name);
      if (kind == im::U_NOM) CHECK(q.dst - rec >= (size_t)n && q.dst - rec < (size_t)n + 4, "%s: u_nom outside n..n+4", L.name);
      if (kind == im::GAIN) CHECK(q.dst - gain < (size_t)(4 * n), "%s: gain outside the dense words", L.name);
      if (kind == im::ZGAIN) CHECK(q.dst - gain < (size_t)mc::KW, "%s: zero gain outside the 56", L.name);
      if (in_traj)
        CHECK(traj_dst.insert(q.dst).second, "%s kind %d: element %ld repeats a destination", L.name, kind, e);
      else
        CHECK(gain_dst.insert(q.dst).second, "%s kind %d: element %ld repeats a destination", L.name, kind, e);
    }
    for (long e = 0; e < blk; ++e) CHECK(hits[(size_t)e] == 1, "%s kind %d: element %ld classified %d times", L.name, kind, e, hits[(size_t)e]);
    CHECK(live == want_live && live > 0, "%s kind %d: %ld destinations, want %ld", L.name, kind, live, want_live);
    if (kind == im::ZGAIN) CHECK(live == (long)nv * 56, "%s: %ld zero gains for %d rows", L.name, live, nv);
    if (kind == im::U_NOM) CHECK(live == (long)nv * 4, "%s: %ld controls for %d rows", L.name, live, nv);
  }
  // nothing outside the listed problem's nominal slot, nothing written twice
  double total = 0;
  for (size_t i = 0; i < traj.size(); ++i) {
    total += traj[i];
    const size_t lo = mc::nom_off(NK, nslot, b, slot, 0), hi = mc::nom_off(NK, nslot, b, slot, NK);
    if (i < lo || i >= hi) CHECK(traj[i] == 0.0, "%s: trajectory element %zu outside the nominal slot written", L.name, i);
    CHECK(traj[i] <= 1.0, "%s: trajectory element %zu written twice", L.name, i);
  }
  CHECK(total == (double)traj_dst.size(), "%s: trajectory writes", L.name);
  for (size_t i = 0; i < K.size(); ++i)
    if (i < mc::gain_off(NK, b, 0) || i >= mc::gain_off(NK, b, NK)) CHECK(K[i] == 0.0, "%s: gain element %zu of another problem written", L.name, i);
}

static void check_layout(const Lay& L) {
  for (int scope : {im::STEPS_CONTROL, im::STEPS_ALL}) {
    const int nph = im::n_phases(scope, L.P, L.n_wb);
    const int ns = im::n_steps(scope, L.P, L.n_wb, L.N.data());
    for (int r : {14, 6}) {
      if (r == 6 && L.n_wb > 0) continue;  // rows of 6 belong to handles whose problems are all SRB-only
      check_window(L, scope, r, 0, 1);
      check_window(L, scope, r, ns - 1, 1);
      int off = 0;
      for (int p = 0; p < nph; ++p) {  // 3 steps before the end of each phase, W = 5
        off += L.N[p] - 1;
        if (off - 3 >= 0 && off - 3 < ns) check_window(L, scope, r, off - 3, 5);
      }
      check_window(L, scope, r, ns > 2 ? ns - 2 : 0, 6);  // past the last step
      check_window(L, scope, r, 0, ns);                   // all steps
      check_window(L, scope, r, 0, ns + 7);
    }
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
  {  // the stated numbers
    const Lay& L = lays[0];
    const im::Lay ml = {L.P, L.n_wb, L.N.data(), L.ko.data()};
    const im::Dims D = {260, 3};
    CHECK(im::n_steps(im::STEPS_CONTROL, 4, 2, L.N.data()) == 158 && im::n_steps(im::STEPS_ALL, 4, 2, L.N.data()) == 256,
          "c3: steps");
    CHECK(im::n_steps(im::STEPS_CONTROL, 3, 0, lays[1].N.data()) == 79 && im::n_steps(im::STEPS_ALL, 3, 0, lays[1].N.data()) == 79,
          "srb-only: both scopes count all phases");
    CHECK(!im::scope_ok(2) && !im::scope_ok(-1) && im::scope_ok(0) && im::scope_ok(1), "scope_ok");
    // C3, first 76, W 5: knots 76, 77, 78 of phase 0, then 0, 1 of phase 1 at kk 80, 81 -- never kk 79
    const int kk_want[5] = {76, 77, 78, 80, 81};
    for (int w = 0; w < 5; ++w) {
      const im::Elem q = im::elem(im::STEPS_ALL, im::U_NOM, 14, ml, D, 0, 0, 76, 5, (long)w * 4);
      CHECK(!q.skip && q.dst == (size_t)kk_want[w] * 24 + 14 && q.phase == (w < 3 ? 0 : 1), "c3: window row %d at %zu", w, q.dst);
    }
    // STEPS_ALL across the whole-body / SRB boundary at step 158: step 157 is kk 158 (n = 14),
    // step 158 is knot 0 of phase 2 at kk 160 (n = 6) -- never kk 159; u_nom at entry 6 there
    const im::Elem a = im::elem(im::STEPS_ALL, im::U_NOM, 14, ml, D, 0, 0, 156, 5, 1 * 4 + 2);
    const im::Elem c = im::elem(im::STEPS_ALL, im::U_NOM, 14, ml, D, 0, 0, 156, 5, 2 * 4 + 2);
    CHECK(!a.skip && a.phase == 1 && a.dst == (size_t)158 * 24 + 14 + 2, "c3: step 157");
    CHECK(!c.skip && c.phase == 2 && c.dst == (size_t)160 * 24 + 6 + 2, "c3: step 158");
    // ... its x_nom uses 6 columns of the 14, its K 4 rows of 6 dense words
    CHECK(!im::elem(im::STEPS_ALL, im::X_NOM, 14, ml, D, 0, 0, 156, 5, 2 * 14 + 5).skip &&
              im::elem(im::STEPS_ALL, im::X_NOM, 14, ml, D, 0, 0, 156, 5, 2 * 14 + 6).skip,
          "c3: an SRB step reads 6 columns of x_nom");
    const im::Elem g = im::elem(im::STEPS_ALL, im::GAIN, 14, ml, D, 0, 0, 156, 5, 2 * 56 + 3 * 14 + 5);
    CHECK(!g.skip && g.dst == (size_t)160 * 56 + 3 * 6 + 5, "c3: an SRB step's gain row 3 column 5");
    CHECK(im::elem(im::STEPS_ALL, im::GAIN, 14, ml, D, 0, 0, 156, 5, 2 * 56 + 3 * 14 + 6).skip, "c3: an SRB step's gain column 6");
    // STEPS_CONTROL stops at step 158
    CHECK(im::elem(im::STEPS_CONTROL, im::U_NOM, 14, ml, D, 0, 0, 156, im::valid(158, 156, 5), 2 * 4).skip,
          "c3: the control scope has no step 158");
    // the rotated layout: step 79 is phase 1 at kk 0
    const Lay& R = lays[3];
    const im::Lay mr = {R.P, R.n_wb, R.N.data(), R.ko.data()};
    const im::Elem q = im::elem(im::STEPS_ALL, im::X_NOM, 14, mr, D, 1, 2, 77, 4, 2 * 14 + 3);
    CHECK(!q.skip && q.phase == 1 && q.dst == (((size_t)1 * 3 + 2) * 260 + 0) * 24 + 3, "rotated: step 79");
  }
  if (fails) {
    std::printf("%d failure(s)\n", fails);
    return 1;
  }
  std::printf("import_map_hostcheck: %zu layouts, %ld elements ok\n", lays.size(), checked);
  return 0;
}
