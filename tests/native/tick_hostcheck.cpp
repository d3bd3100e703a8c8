// Host check of the solve scope (csrc/mhpc_plan.h: solve_scope, scope_clip, scope_split), the pure
// part of mhpc_tick_problems' plan: plain g++, no HIP, no handle.  Synthetic plans of a few
// problems; "ok" and exit status 0 when every check holds, the first violated checks otherwise.
//
//  * a list spanning several groups with one group that has no listed problem, worked by hand;
//  * n = 1;
//  * the list equal to the whole batch (in plan order and shuffled): the plan's own go[] / gidx;
//  * an unsorted list: the order is by group, then problem number, whatever the list's order;
//  * the fresh / rolled split with all, none and some of the listed problems fresh;
//  * sub-batch clipping with a block that ends inside a group, and the split of a clipped block;
//  * over random plans and lists: order a permutation of the list, grouped and ascending, go[] its
//    group counts, split = rolled-out problems then fresh ones, each in order, and the clipped
//    halves of an even partition tile both halves of split exactly.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_plan.h"

using namespace MHPC_NS;

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

uint64_t rng_state = 0x5449434B;
int rnd(int n) {  // 0..n-1
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (int)((rng_state >> 33) % (uint64_t)n);
}

// A layout of one whole-body phase of N knots (distinct N: distinct layouts, longest first)
ProbLayout lay(int N) {
  ProbLayout q;
  memset(&q, 0, sizeof q);
  q.desc.n_wb = 1;
  q.desc.mode_seq[0] = 1;
  q.desc.N[0] = N;
  q.desc.dt_wb = 0.001;
  q.desc.dt_fb = 0.002;
  q.desc.precision = 64;
  return q;
}
// Problem b on layout of N[b] knots and set set_of[b]
GroupPlan make_plan(const std::vector<int>& N, const std::vector<int>& set_of) {
  std::vector<ProbLayout> pl;
  for (int n : N) pl.push_back(lay(n));
  GroupPlan plan;
  const char* msg = nullptr;
  const int rc = plan_groups(pl, set_of, plan, &msg);
  CHECK(rc == MHPC_OK, "%s", msg ? msg : "");
  return plan;
}
bool eq(const std::vector<int>& a, std::initializer_list<int> b) { return a == std::vector<int>(b); }
bool eq_go(const int* go, std::initializer_list<int> b) { return std::equal(b.begin(), b.end(), go); }

// 8 problems, 4 groups: knots 5 (problems 1, 6), 4 (0, 3, 7), 3 (2), 2 (4, 5)
GroupPlan hand_plan() {
  const GroupPlan plan = make_plan({4, 5, 3, 4, 2, 2, 5, 4}, std::vector<int>(8, 0));
  CHECK(plan.ngrp == 4, "%d", plan.ngrp);
  CHECK(eq(plan.gidx, {1, 6, 0, 3, 7, 2, 4, 5}), "gidx");
  return plan;
}

void hand_cases() {
  const GroupPlan plan = hand_plan();
  {  // several groups, group 2 (problem 2) without a listed problem; the list unsorted
    const SolveScope s = solve_scope(plan, {7, 4, 1, 0}, {});
    CHECK(eq(s.order, {1, 0, 7, 4}), "order");
    CHECK(s.ngrp == 4 && eq_go(s.go, {0, 1, 3, 3, 4}), "go %d %d %d %d %d", s.go[0], s.go[1], s.go[2], s.go[3], s.go[4]);
    CHECK(s.nnf == 4 && eq(s.split, {1, 0, 7, 4}) && eq(s.nf, {0, 1, 2, 3, 4}), "no fresh: split is order");
    // the same problems in another order: the same scope
    const SolveScope t = solve_scope(plan, {0, 1, 4, 7}, {});
    CHECK(t.order == s.order && std::equal(s.go, s.go + MAXL + 1, t.go), "list order does not matter");
  }
  {  // n = 1
    const SolveScope s = solve_scope(plan, {2}, {});
    CHECK(eq(s.order, {2}) && eq_go(s.go, {0, 0, 0, 1, 1}), "n = 1");
    CHECK(s.nnf == 1 && eq(s.split, {2}) && eq(s.nf, {0, 1}), "n = 1 split");
    std::vector<char> fresh(8, 0);
    fresh[2] = 1;
    const SolveScope f = solve_scope(plan, {2}, fresh);
    CHECK(f.nnf == 0 && eq(f.split, {2}) && eq(f.nf, {0, 0}), "n = 1 fresh");
    int gof[MAXL + 1], goc[MAXL + 1];
    scope_split(f, f.go, gof, goc);
    CHECK(eq_go(gof, {0, 0, 0, 0, 0}) && eq_go(goc, {0, 0, 0, 1, 1}), "n = 1 fresh halves");
  }
  {  // the whole batch: the plan's own gidx / go[], from any order of the list
    const SolveScope s = solve_scope(plan, plan.gidx, {});
    CHECK(s.order == plan.gidx && std::equal(plan.go, plan.go + MAXL + 1, s.go), "whole batch");
    const SolveScope t = solve_scope(plan, {5, 2, 7, 0, 3, 6, 1, 4}, {});
    CHECK(t.order == plan.gidx && std::equal(plan.go, plan.go + MAXL + 1, t.go), "whole batch, shuffled");
  }
  {  // fresh / rolled split: some, all, none of the listed problems fresh (an unlisted fresh one
     // does not count)
    std::vector<char> fresh(8, 0);
    fresh[0] = fresh[4] = fresh[6] = 1;  // 6 is not listed below
    const std::vector<int> list = {7, 4, 1, 0, 5};
    const SolveScope s = solve_scope(plan, list, fresh);
    CHECK(eq(s.order, {1, 0, 7, 4, 5}) && eq_go(s.go, {0, 1, 3, 3, 5}), "order with fresh");
    CHECK(s.nnf == 3 && eq(s.split, {1, 7, 5, 0, 4}) && eq(s.nf, {0, 1, 1, 2, 2, 3}), "some fresh");
    int gof[MAXL + 1], goc[MAXL + 1];
    scope_split(s, s.go, gof, goc);
    CHECK(eq_go(gof, {0, 1, 2, 2, 3}) && eq_go(goc, {3, 3, 4, 4, 5}), "some fresh: halves");
    const SolveScope a = solve_scope(plan, list, std::vector<char>(8, 1));
    CHECK(a.nnf == 0 && a.split == a.order, "all fresh");
    scope_split(a, a.go, gof, goc);
    CHECK(eq_go(gof, {0, 0, 0, 0, 0}) && eq_go(goc, {0, 1, 3, 3, 5}), "all fresh: halves");
    const SolveScope z = solve_scope(plan, list, std::vector<char>(8, 0));
    CHECK(z.nnf == 5 && z.split == z.order, "none fresh");
    scope_split(z, z.go, gof, goc);
    CHECK(eq_go(gof, {0, 1, 3, 3, 5}) && eq_go(goc, {5, 5, 5, 5, 5}), "none fresh: halves");
    // sub-batch clipping: two blocks of positions [0, 2) and [2, 5); the first ends inside group 1
    int c0[MAXL + 1], c1[MAXL + 1];
    scope_clip(s.go, s.ngrp, 0, 2, c0);
    scope_clip(s.go, s.ngrp, 2, 5, c1);
    CHECK(eq_go(c0, {0, 1, 2, 2, 2}) && eq_go(c1, {2, 2, 3, 3, 5}), "clip");
    scope_split(s, c0, gof, goc);  // positions 0, 1: problem 1 rolled out, problem 0 fresh
    CHECK(eq_go(gof, {0, 1, 1, 1, 1}) && eq_go(goc, {3, 3, 4, 4, 4}), "clipped halves, block 0");
    scope_split(s, c1, gof, goc);  // positions 2..4: 7 and 5 rolled out, 4 fresh
    CHECK(eq_go(gof, {1, 1, 2, 2, 3}) && eq_go(goc, {4, 4, 4, 4, 5}), "clipped halves, block 1");
  }
}

void random_cases() {
  for (int it = 0; it < 300; ++it) {
    const int B = 1 + rnd(40), nl = 1 + rnd(5), nsets = 1 + rnd(3);
    std::vector<int> N(B), set_of(B);
    for (int b = 0; b < B; ++b) {
      N[b] = 2 + rnd(nl);
      set_of[b] = rnd(nsets);
    }
    const GroupPlan plan = make_plan(N, set_of);
    std::vector<int> all(B);
    for (int b = 0; b < B; ++b) all[b] = b;
    for (int i = B - 1; i > 0; --i) std::swap(all[i], all[rnd(i + 1)]);
    const int n = 1 + rnd(B);
    const std::vector<int> list(all.begin(), all.begin() + n);
    std::vector<char> fresh(B);
    const int mode = rnd(3);
    for (int b = 0; b < B; ++b) fresh[b] = mode == 0 ? 0 : mode == 1 ? 1 : (char)rnd(2);
    const SolveScope s = solve_scope(plan, list, fresh);
    CHECK(s.size() == n && s.ngrp == plan.ngrp, "size");
    std::vector<int> a = s.order, l = list;
    std::sort(a.begin(), a.end());
    std::sort(l.begin(), l.end());
    CHECK(a == l, "order is a permutation of the list");
    CHECK(s.go[0] == 0 && s.go[plan.ngrp] == n, "go ends");
    for (int g = 0; g < plan.ngrp; ++g) {
      CHECK(s.go[g] <= s.go[g + 1], "go monotone");
      for (int pos = s.go[g]; pos < s.go[g + 1]; ++pos) {
        CHECK(plan.lid[s.order[pos]] == g, "position %d in group %d", pos, g);
        CHECK(pos == s.go[g] || s.order[pos - 1] < s.order[pos], "ascending inside a group");
      }
    }
    // split: the rolled-out problems in order, then the fresh ones in order
    std::vector<int> want, tail;
    for (int b : s.order) (fresh[b] ? tail : want).push_back(b);
    CHECK(s.nnf == (int)want.size(), "nnf");
    want.insert(want.end(), tail.begin(), tail.end());
    CHECK(s.split == want, "split");
    // an even partition into blocks: the blocks' halves tile [0, nnf) and [nnf, n) group by group,
    // and each half's ranges hold exactly the block's problems of that kind, grouped
    const int nsub = 1 + rnd(std::min(n, 4));
    std::vector<char> seen(B, 0);
    for (int k = 0; k < nsub; ++k) {
      const int b0 = (int)((int64_t)k * n / nsub), b1 = (int)((int64_t)(k + 1) * n / nsub);
      int c[MAXL + 1], gof[MAXL + 1], goc[MAXL + 1];
      scope_clip(s.go, s.ngrp, b0, b1, c);
      CHECK(c[0] == b0 && c[s.ngrp] == b1, "clip ends");
      scope_split(s, c, gof, goc);
      for (int g = 0; g < s.ngrp; ++g) {
        CHECK(gof[g + 1] - gof[g] + goc[g + 1] - goc[g] == c[g + 1] - c[g], "halves add up");
        for (int half = 0; half < 2; ++half) {
          const int* go = half ? goc : gof;
          CHECK(go[g] >= (half ? s.nnf : 0) && go[g + 1] <= (half ? n : s.nnf), "half in its range");
          for (int pos = go[g]; pos < go[g + 1]; ++pos) {
            const int b = s.split[pos];
            CHECK(plan.lid[b] == g && (fresh[b] != 0) == (half != 0), "split position %d", pos);
            CHECK(!seen[b], "problem %d in two blocks", b);
            seen[b] = 1;
          }
        }
      }
    }
    int nseen = 0;
    for (int b = 0; b < B; ++b) nseen += seen[b];
    CHECK(nseen == n, "every listed problem in one block's half: %d of %d", nseen, n);
  }
}
}  // namespace

int main() {
  hand_cases();
  random_cases();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
