// Host check of what the calls on some problems of a live batch share (csrc/mhpc_plan.h:
// ProblemList, pack_rows, solve_scope as mhpc_reset_problems uses it, Ledger): plain
// g++, no HIP, no handle.  Synthetic batches of 4 to 8 problems; "ok" and exit status 0 when every
// check holds, the first violated checks otherwise.
//
//  * the problem list: n = 0, n = B + 1, an index of -1, an index of B, a duplicate at the first and
//    at the last place, each with its exact message in both wordings;
//    a valid shuffled list gives each problem's place;
//  * the row packer on a batch that mixes whole-body and SRB-only problems (caller rows of 14) and
//    on one of SRB-only problems (rows of 6), one and three samples a problem, rows taken in range
//    order, list order and group order (through at[]): every entry against an indexing written out
//    here, the padding zero, the tail of an SRB-only problem's caller row (NaN here) never copied.
//    The caller's array ends with the 6th entry of the last row, so the sanitized build also shows
//    that nothing past an SRB-only problem's entries is read;
//  * mhpc_reset_problems' order and go[]: over random plans and lists, solve_scope with no fresh
//    problem against the sort and the count the runtime had of its own (kept here as the reference);
//  * the ledger against the members it replaced (fresh / nfresh, cmd_mark / ncmd / cmd_changed,
//    srb_open, edited in place exactly as the runtime did, kept here as `Old`): after every
//    transition of random sequences over 6 problems in two handles every flag, count and "any
//    command mark" agree, each count is the number of set flags, and cmd_changed == ncmd > 0;
//  * the ledger's hand-worked cases: initialize with one record without AL iterations; reset then a
//    gait step; a tick of two problems; a copy inside one ledger between problems whose flags
//    differ; the budget-raise rule right after initialize, after a solve, and with the rollout due.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <memory>
#include <string>
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

uint64_t rng_state = 0x4C454447;
int rnd(int n) {  // 0..n-1
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (int)((rng_state >> 33) % (uint64_t)n);
}
std::vector<int> shuffled(int B) {
  std::vector<int> all(B);
  for (int b = 0; b < B; ++b) all[b] = b;
  for (int i = B - 1; i > 0; --i) std::swap(all[i], all[rnd(i + 1)]);
  return all;
}

// ---- the problem list -----------------------------------------------------------------------------
const char* kN[2] = {"n must be 1..batch", "n must be 1..batch of the destination"};
const char* kRange = "problem out of range";
const char* kTwice[2] = {"problem listed twice", "destination problem listed twice"};

// A whole list through ProblemList, as the runtime's callers run it; at: left alone by a refusal
int check_list(int n, const int* problems, int B, bool copy, std::vector<int>& at, const char** msg) {
  ProblemList l;
  int rc = l.begin(n, B, copy, msg);
  for (int i = 0; !rc && i < n; ++i) rc = l.add(problems[i], msg);
  if (!rc) CHECK(l.n == n, "entries counted: %d", l.n);
  if (!rc) at.swap(l.at);
  return rc;
}
void list_case(const std::vector<int>& list, int n, int B, bool copy, const char* want) {
  const std::vector<int> before = {7, 7, 7};
  std::vector<int> at = before;
  const char* msg = nullptr;
  const int rc = check_list(n, list.data(), B, copy, at, &msg);
  CHECK((rc == MHPC_OK) == !want, "rc %d", rc);
  if (want) {
    CHECK(rc == MHPC_ERR_INVALID && msg && !strcmp(msg, want), "'%s' for '%s'", msg ? msg : "", want);
    CHECK(at == before, "a refusal leaves at alone");
  } else {
    CHECK((int)at.size() == B, "at has one entry a problem");
    std::vector<int> exp(B, -1);
    for (int i = 0; i < n; ++i) exp[list[i]] = i;
    CHECK(at == exp, "places");
  }
}
void list_cases() {
  const int B = 6;
  for (int copy = 0; copy < 2; ++copy) {
    list_case({0}, 0, B, copy, kN[copy]);
    list_case({0, 1, 2, 3, 4, 5, 0}, B + 1, B, copy, kN[copy]);
    list_case({2, -1, 3}, 3, B, copy, kRange);
    list_case({2, B, 3}, 3, B, copy, kRange);
    list_case({3, 3, 1}, 3, B, copy, kTwice[copy]);     // the first place a duplicate can be
    list_case({0, 4, 2, 0}, 4, B, copy, kTwice[copy]);  // the last entry repeats the first
    list_case({5, 4, 2, 2}, 4, B, copy, kTwice[copy]);  // ... the one before it
    list_case({-1, -1}, 2, B, copy, kRange);            // out of range before twice
    list_case({4}, 1, B, copy, nullptr);
    list_case({4, 0, 5, 2}, 4, B, copy, nullptr);
    for (int it = 0; it < 20; ++it) {
      const int Bi = 4 + rnd(5);
      list_case(shuffled(Bi), 1 + rnd(Bi), Bi, copy, nullptr);
    }
  }
}

// ---- plans ----------------------------------------------------------------------------------------
// wb: one whole-body phase and one SRB phase; else two SRB phases.  N: knots of the first phase
// (distinct N: distinct layouts, longest first)
ProbLayout lay(bool wb, int N) {
  ProbLayout q;
  memset(&q, 0, sizeof q);
  q.desc.n_wb = wb ? 1 : 0;
  q.desc.n_fb = wb ? 1 : 2;
  q.desc.mode_seq[0] = 1;
  q.desc.mode_seq[1] = 2;
  q.desc.N[0] = N;
  q.desc.N[1] = 2;
  q.desc.dt_wb = 0.001;
  q.desc.dt_fb = 0.002;
  q.desc.precision = 64;
  return q;
}
GroupPlan make_plan(const std::vector<ProbLayout>& pl, const std::vector<int>& set_of) {
  GroupPlan plan;
  const char* msg = nullptr;
  const int rc = plan_groups(pl, set_of, plan, &msg);
  CHECK(rc == MHPC_OK, "%s", msg ? msg : "");
  return plan;
}

// ---- the row packer -------------------------------------------------------------------------------
// Destination row j of problem prob[j] from caller row from[j]: every entry of pack_rows' output
// against this indexing.  The caller's array is exactly as long as pack_rows may read: it ends with
// the last entry of the last row's problem.
template <class E>
void pack_case(const GroupPlan& plan, const std::vector<char>& wb, int n_s, int first,
               const std::vector<int>& prob, const std::vector<int>& from, bool by_prob, bool by_at) {
  const int count = (int)prob.size();
  bool any = false;
  for (char w : wb) any = any || w;
  const int r = any ? 14 : 6;
  CHECK(x0_row_of(plan) == r, "row width %d", x0_row_of(plan));
  int nrows = 0, last_w = r;
  for (int j = 0; j < count; ++j)
    if (from[j] + 1 > nrows) {
      nrows = from[j] + 1;
      last_w = wb[prob[j]] ? 14 : 6;
    }
  const size_t len = ((size_t)nrows * n_s - 1) * r + last_w;
  std::unique_ptr<double[]> src(new double[len]);
  for (size_t i = 0; i < len; ++i) src[i] = 1.0 + (double)i / 3.0;
  // the tail of an SRB-only problem's caller row: never to be copied
  for (int j = 0; j < count; ++j)
    if (!wb[prob[j]])
      for (int t = 0; t < n_s; ++t)
        for (int i = 6; i < r; ++i) {
          const size_t o = ((size_t)from[j] * n_s + t) * r + i;
          if (o < len) src[o] = std::numeric_limits<double>::quiet_NaN();
        }
  std::vector<int> at(wb.size(), -1);
  for (int j = 0; j < count; ++j) at[prob[j]] = from[j];
  const std::vector<E> out = pack_rows<E>(plan, count, n_s, src.get(), first, by_prob ? prob.data() : nullptr,
                                          by_at ? at.data() : nullptr);
  CHECK(out.size() == (size_t)count * n_s * 14, "size %zu", out.size());
  for (int j = 0; j < count; ++j)
    for (int t = 0; t < n_s; ++t)
      for (int i = 0; i < 14; ++i) {
        const int w = wb[prob[j]] ? 14 : 6;
        const E want = i < w ? (E)src[((size_t)from[j] * n_s + t) * r + i] : E(0);
        const E got = out[((size_t)j * n_s + t) * 14 + i];
        CHECK(got == want, "row %d sample %d entry %d: %g, want %g", j, t, i, (double)got, (double)want);
      }
}
template <class E>
void pack_cases() {
  // 7 problems: whole-body ones 0, 3, 4, 6 (knots 4, 5, 4, 3), SRB-only ones 1, 2, 5 (knots 3, 6, 3)
  const std::vector<char> mixed = {1, 0, 0, 1, 1, 0, 1}, srb(5, 0);
  const std::vector<int> Nm = {4, 3, 6, 5, 4, 3, 3}, Ns = {2, 3, 3, 4, 2};
  for (int which = 0; which < 2; ++which) {
    const std::vector<char>& wb = which ? srb : mixed;
    const std::vector<int>& N = which ? Ns : Nm;
    const int B = (int)wb.size();
    std::vector<ProbLayout> pl;
    for (int b = 0; b < B; ++b) pl.push_back(lay(wb[b], N[b]));
    CHECK(x0_row_of(pl) == (which ? 6 : 14), "row width of the layouts");
    const GroupPlan plan = make_plan(pl, std::vector<int>(B, 0));
    CHECK(!plan.ident, "the plan regroups the batch");
    for (int n_s : {1, 3}) {
      // range order: the whole batch, and a range that ends on an SRB-only problem
      for (auto range : {std::pair<int, int>(0, B), std::pair<int, int>(1, which ? 3 : 5)}) {
        std::vector<int> prob, from;
        for (int j = 0; j < range.second; ++j) {
          prob.push_back(range.first + j);
          from.push_back(j);
        }
        pack_case<E>(plan, wb, n_s, range.first, prob, from, false, false);
      }
      // list order: the caller's rows are the list's; group order: the scope's order, each row
      // from its problem's place in the list
      for (const std::vector<int>& list : {std::vector<int>{4, 1, 3, 2}, std::vector<int>{2}, shuffled(B)}) {
        std::vector<int> from(list.size());
        for (size_t j = 0; j < list.size(); ++j) from[j] = (int)j;
        pack_case<E>(plan, wb, n_s, 0, list, from, true, false);
        std::vector<int> at;
        const char* msg = nullptr;
        CHECK(check_list((int)list.size(), list.data(), B, false, at, &msg) == MHPC_OK, "list");
        const SolveScope ss = solve_scope(plan, list, {});
        for (size_t j = 0; j < list.size(); ++j) from[j] = at[ss.order[j]];
        pack_case<E>(plan, wb, n_s, 0, ss.order, from, true, true);
      }
    }
  }
}

// ---- mhpc_reset_problems' order and go[] ------------------------------------------------------------
void reset_scope_cases() {
  for (int it = 0; it < 300; ++it) {
    const int B = 4 + rnd(5), nsets = 1 + rnd(3);
    std::vector<ProbLayout> pl;
    std::vector<int> set_of(B);
    for (int b = 0; b < B; ++b) {
      pl.push_back(lay(rnd(2), 2 + rnd(4)));
      set_of[b] = rnd(nsets);
    }
    const GroupPlan plan = make_plan(pl, set_of);
    const std::vector<int> all = shuffled(B);
    const int n = 1 + rnd(B);
    const std::vector<int> list(all.begin(), all.begin() + n);
    // the runtime's own sort (api_reset_problems) and count (reset_launches) before solve_scope
    // served them
    std::vector<int> order(list);
    std::sort(order.begin(), order.end(), [&](int a, int c) {
      return plan.lid[a] != plan.lid[c] ? plan.lid[a] < plan.lid[c] : a < c;
    });
    int go[MAXL + 1] = {};
    for (int b : order) ++go[plan.lid[b] + 1];
    for (int g = 0; g < plan.ngrp; ++g) go[g + 1] += go[g];
    const SolveScope ss = solve_scope(plan, list, {});
    CHECK(ss.order == order, "order");
    CHECK(ss.ngrp == plan.ngrp && std::equal(go, go + plan.ngrp + 1, ss.go), "go");
    CHECK(ss.nnf == n && ss.split == order, "no fresh problem: nothing to split");
  }
}

// ---- the ledger -------------------------------------------------------------------------------------
// The handle's call-order flags the budget rule reads
struct Flags {
  bool need_full = false, solved = false, initialized = false;
};
// The members the ledger replaced, edited in place as the runtime edited them.
struct Old : Flags {
  std::vector<char> fresh, cmd_mark, srb_open;
  int nfresh = 0, ncmd = 0;
  bool cmd_changed = false;
  explicit Old(int B) : fresh(B, 0), cmd_mark(B, 0), srb_open(B, 0) {}
  void mark_current() {
    cmd_changed = false;
    std::fill(cmd_mark.begin(), cmd_mark.end(), 0);
    ncmd = 0;
    solved = false;
  }
  void initialize(const std::vector<char>& no_al) {
    need_full = false;
    std::fill(fresh.begin(), fresh.end(), 0);
    nfresh = 0;
    for (size_t b = 0; b < fresh.size(); ++b) srb_open[b] = no_al[b];
    initialized = true;
    mark_current();
  }
  void solve() {
    solved = true;
    need_full = false;
    std::fill(fresh.begin(), fresh.end(), 0);
    nfresh = 0;
    std::fill(srb_open.begin(), srb_open.end(), 0);
  }
  void tick(const std::vector<int>& list) {
    for (int b : list) {
      if (fresh[b]) {
        fresh[b] = 0;
        --nfresh;
      }
      srb_open[b] = 0;
      if (cmd_mark[b]) {
        cmd_mark[b] = 0;
        --ncmd;
      }
    }
    cmd_changed = ncmd > 0;
  }
  void update(const std::vector<int>& steps) {
    for (size_t b = 0; b < fresh.size(); ++b)
      if (fresh[b] && steps[b] > 0) {
        fresh[b] = 0;
        --nfresh;
      }
    need_full = true;
    mark_current();
  }
  void reset(const std::vector<int>& list, const std::vector<char>& no_al) {
    for (int b : list) {
      if (!fresh[b]) {
        fresh[b] = 1;
        ++nfresh;
      }
      srb_open[b] = no_al[b];
    }
  }
  void copy(int b, const Old& s, int a) {
    nfresh += (s.fresh[a] ? 1 : 0) - (fresh[b] ? 1 : 0);
    fresh[b] = s.fresh[a];
    srb_open[b] = s.srb_open[a];
  }
  void commands(const std::vector<int>& changed) {
    if (initialized) {
      for (int b : changed)
        if (!cmd_mark[b]) {
          cmd_mark[b] = 1;
          ++ncmd;
        }
      cmd_changed = ncmd > 0;
    }
  }
  void options(const std::vector<int>& changed, const std::vector<char>& no_al) {
    const int B = (int)fresh.size();
    for (int b : changed) {
      if (!srb_open[b] || no_al[b]) continue;
      srb_open[b] = 0;
      if (!need_full && !solved && initialized) {
        need_full = true;
        for (int q = 0; q < B; ++q) fresh[q] = 1;
        nfresh = B;
      }
      if (fresh[b]) {
        fresh[b] = 0;
        --nfresh;
      }
    }
  }
  void set_layouts() { initialized = solved = false; }
};
// The same events as the runtime spells them with the ledger.
struct New : Flags {
  Ledger led;
  explicit New(int B) : led(B) {}
  void mark_current() {
    led.all_current();
    solved = false;
  }
  void initialize(const std::vector<char>& no_al) {
    need_full = false;
    led.initialized([&](int b) { return no_al[b] != 0; });
    initialized = true;
    mark_current();
  }
  void solve() {
    solved = true;
    need_full = false;
    led.solved();
  }
  void tick(const std::vector<int>& list) { led.ticked((int)list.size(), list.data()); }
  void update(const std::vector<int>& steps) {
    for (int b = 0; b < led.size(); ++b)
      if (steps[b] > 0) led.stepped(b);
    need_full = true;
    mark_current();
  }
  void reset(const std::vector<int>& list, const std::vector<char>& no_al) {
    for (int b : list) led.reset(b, no_al[b]);
  }
  void copy(int b, const New& s, int a) { led.copied(b, s.led, a); }
  void commands(const std::vector<int>& changed) {
    if (initialized)
      for (int b : changed) led.command_changed(b);
  }
  void options(const std::vector<int>& changed, const std::vector<char>& no_al) {
    for (int b : changed)
      if (!no_al[b] && led.budget_raised(b, !need_full && !solved && initialized)) need_full = true;
  }
  void set_layouts() { initialized = solved = false; }
};

int count(const std::vector<char>& f) { return (int)std::count_if(f.begin(), f.end(), [](char c) { return c != 0; }); }
void same(const Old& o, const New& n, const char* after) {
  const int B = n.led.size();
  int nf = 0, nm = 0;
  for (int b = 0; b < B; ++b) {
    CHECK(n.led.fresh(b) == (o.fresh[b] != 0), "fresh[%d] after %s", b, after);
    CHECK(n.led.open(b) == (o.srb_open[b] != 0), "open[%d] after %s", b, after);
    CHECK(n.led.marked(b) == (o.cmd_mark[b] != 0), "mark[%d] after %s", b, after);
    CHECK(n.led.fresh_flags()[b] == o.fresh[b], "fresh_flags[%d] after %s", b, after);
    nf += n.led.fresh(b);
    nm += n.led.marked(b);
  }
  CHECK(n.led.nfresh() == nf && nf == o.nfresh, "nfresh %d, flags %d, old %d after %s", n.led.nfresh(), nf, o.nfresh, after);
  CHECK(n.led.nmarked() == nm && nm == o.ncmd, "ncmd %d, flags %d, old %d after %s", n.led.nmarked(), nm, o.ncmd, after);
  CHECK(n.led.cmd_pending() == (nm > 0), "any command mark after %s", after);
  // the stored flag the ledger no longer has: the same as "any mark" on every path
  CHECK(o.cmd_changed == (o.ncmd > 0) && o.ncmd == count(o.cmd_mark), "cmd_changed == ncmd > 0 after %s", after);
  CHECK(o.nfresh == count(o.fresh), "old nfresh after %s", after);
  CHECK(o.need_full == n.need_full && o.solved == n.solved && o.initialized == n.initialized, "flags after %s", after);
}

std::vector<int> some(int B, bool may_be_empty) {
  const std::vector<int> all = shuffled(B);
  const int n = may_be_empty ? rnd(B + 1) : 1 + rnd(B);
  return std::vector<int>(all.begin(), all.begin() + n);
}
std::vector<char> flags(int B) {
  std::vector<char> f(B);
  for (char& c : f) c = (char)(rnd(3) == 0);
  return f;
}
void ledger_random() {
  const int B = 6;
  for (int seq = 0; seq < 40; ++seq) {
    Old o[2] = {Old(B), Old(B)};
    New n[2] = {New(B), New(B)};
    for (int step = 0; step < 300; ++step) {
      const int k = rnd(2), ev = rnd(10);
      const char* name = "";
      switch (ev) {
        case 0: {
          const std::vector<char> na = flags(B);
          o[k].initialize(na), n[k].initialize(na), name = "initialize";
          break;
        }
        case 1:
          o[k].solve(), n[k].solve(), name = "solve";
          break;
        case 2: {
          const std::vector<int> l = some(B, false);
          o[k].tick(l), n[k].tick(l), name = "tick";
          break;
        }
        case 3: {
          std::vector<int> st(B);
          for (int& s : st) s = rnd(3);
          o[k].update(st), n[k].update(st), name = "update";
          break;
        }
        case 4: {
          const std::vector<int> l = some(B, false);
          const std::vector<char> na = flags(B);
          o[k].reset(l, na), n[k].reset(l, na), name = "reset";
          break;
        }
        case 5: {  // one handle: a source is no destination; the runtime reads every source's entry
                   // before a later pair writes it, which distinct pairs give here as well
          const std::vector<int> all = shuffled(B);
          const int np = 1 + rnd(B / 2);
          for (int i = 0; i < np; ++i) o[k].copy(all[i], o[k], all[B - 1 - i]), n[k].copy(all[i], n[k], all[B - 1 - i]);
          name = "copy inside a handle";
          break;
        }
        case 6: {
          const std::vector<int> l = some(B, false);
          for (int b : l) {
            const int a = rnd(B);
            o[k].copy(b, o[1 - k], a), n[k].copy(b, n[1 - k], a);
          }
          name = "copy between handles";
          break;
        }
        case 7: {
          const std::vector<int> l = some(B, true);
          o[k].commands(l), n[k].commands(l), name = "set_commands";
          break;
        }
        case 8: {
          std::vector<int> l = some(B, true);
          std::sort(l.begin(), l.end());  // (plan_options: changed is in problem order)
          const std::vector<char> na = flags(B);
          o[k].options(l, na), n[k].options(l, na), name = "set_option_sets";
          break;
        }
        default:
          o[k].set_layouts(), n[k].set_layouts(), name = "set_layouts";
      }
      same(o[0], n[0], name);
      same(o[1], n[1], name);
    }
  }
}

void ledger_hand() {
  const int B = 6;
  auto is = [&](const Ledger& l, std::initializer_list<int> fresh, std::initializer_list<int> open,
                std::initializer_list<int> mark, const char* what) {
    std::vector<char> f(B, 0), o(B, 0), m(B, 0);
    for (int b : fresh) f[b] = 1;
    for (int b : open) o[b] = 1;
    for (int b : mark) m[b] = 1;
    for (int b = 0; b < B; ++b)
      CHECK(l.fresh(b) == (f[b] != 0) && l.open(b) == (o[b] != 0) && l.marked(b) == (m[b] != 0), "%s: problem %d", what, b);
    CHECK(l.nfresh() == (int)fresh.size() && l.nmarked() == (int)mark.size() && l.cmd_pending() == (mark.size() > 0),
          "%s: counts %d %d", what, l.nfresh(), l.nmarked());
  };
  std::vector<char> na(B, 0);
  na[4] = 1;
  {  // initialize with one record without AL iterations: exactly that problem's SRB nominal open
    New h(B);
    is(h.led, {}, {}, {}, "created");
    h.led.reset(1, false);  // (whatever was there before goes)
    h.initialize(na);
    is(h.led, {}, {4}, {}, "initialize");
    // reset makes a problem fresh, a gait step un-freshes it (a step of 0 does not)
    h.solve();
    is(h.led, {}, {}, {}, "solve closes the open nominal");
    h.reset({2, 4}, na);
    is(h.led, {2, 4}, {4}, {}, "reset");
    h.reset({2}, na);
    is(h.led, {2, 4}, {4}, {}, "reset again: counted once");
    h.update({1, 1, 0, 1, 2, 1});
    is(h.led, {2}, {4}, {}, "a gait step un-freshes 4, no step leaves 2");
    CHECK(h.need_full, "update: rollout due");
  }
  {  // a tick clears fresh, open and the command mark of the listed problems only
    New h(B);
    h.initialize(na);
    h.solve();
    h.reset({0, 3, 4}, na);
    h.commands({3, 5, 1});
    is(h.led, {0, 3, 4}, {4}, {1, 3, 5}, "before the tick");
    h.tick({4, 3});
    is(h.led, {0}, {}, {1, 5}, "tick of 4 and 3");
    h.tick({1, 5});
    is(h.led, {0}, {}, {}, "tick of the last marked problems: nothing pending");
  }
  {  // copy inside one ledger: the flags move, the counts follow, also when they differ
    New h(B);
    h.initialize(na);
    h.solve();
    h.reset({0, 4}, na);  // 0: fresh; 4: fresh and open; the others neither
    h.copy(1, h, 0);      // not fresh <- fresh
    is(h.led, {0, 1, 4}, {4}, {}, "copy fresh onto not fresh");
    h.copy(0, h, 2);      // fresh <- not fresh
    is(h.led, {1, 4}, {4}, {}, "copy not fresh onto fresh");
    h.copy(3, h, 4);      // open travels
    is(h.led, {1, 3, 4}, {3, 4}, {}, "copy fresh and open");
    h.copy(4, h, 4);      // onto itself: nothing
    h.copy(1, h, 3);      // fresh <- fresh
    is(h.led, {1, 3, 4}, {1, 3, 4}, {}, "copy fresh onto fresh");
  }
  const std::vector<char> all_al(B, 0);
  {  // budget raised right after initialize: the solve starts with the rollout for 4 and with the
     // cost evaluation for everybody else
    New h(B);
    h.initialize(na);
    h.options({2}, all_al);  // 2 was not open: nothing
    is(h.led, {}, {4}, {}, "raise on a closed problem");
    CHECK(!h.need_full, "raise on a closed problem: no rollout");
    h.options({4}, na);  // its new record still has no AL iteration: nothing
    is(h.led, {}, {4}, {}, "still no AL iteration");
    h.options({4}, all_al);
    is(h.led, {0, 1, 2, 3, 5}, {}, {}, "raise just after initialize: all fresh, then 4 not");
    CHECK(h.need_full, "raise just after initialize: rollout due");
  }
  {  // two open problems raised in one call: the second finds the rollout due already
    std::vector<char> two(B, 0);
    two[1] = two[4] = 1;
    New h(B);
    h.initialize(two);
    h.options({1, 4}, all_al);
    is(h.led, {0, 2, 3, 5}, {}, {}, "two raised at once");
    CHECK(h.need_full, "two raised at once: rollout due");
  }
  {  // after a solve (a reset left 4 open and fresh): the next first sweep is the rollout anyway,
     // 4 only stops being fresh
    New h(B);
    h.initialize(std::vector<char>(B, 0));
    h.solve();
    h.reset({2, 4}, na);
    h.options({4}, all_al);
    is(h.led, {2}, {}, {}, "raise after a solve");
    CHECK(!h.need_full && h.solved, "raise after a solve: flags stay");
  }
  {  // with the rollout due already (an update since the solve)
    New h(B);
    h.initialize(std::vector<char>(B, 0));
    h.solve();
    h.update(std::vector<int>(B, 1));
    h.reset({2, 4}, na);
    h.options({4}, all_al);
    is(h.led, {2}, {}, {}, "raise with the rollout due");
    CHECK(h.need_full, "raise with the rollout due: still due");
  }
}
}  // namespace

int main() {
  list_cases();
  pack_cases<real>();
  pack_cases<double>();
  reset_scope_cases();
  ledger_random();
  ledger_hand();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
