// Host check of the snapshot's staging side and blob layout (csrc/mhpc_snapshot_map.h on top of
// csrc/mhpc_copy_map.h), the code the device path runs: synthetic problems of uniquely tagged
// elements are packed out of handle arrays of knot stride 12 (or 7) into staging buffers of stride
// 7 through run_of / piece_of / width_of, moved to a blob payload array by array as snap_move
// does, in rounds of 3 over 8 entries (3, 3, 2), and unpacked again into handle arrays of stride 7
// and 12, with and without a store on either side, for 8- and 4-byte elements.
//  * the payload equals, byte for byte, the arrays of a handle of stride 7 holding the listed
//    problems in list order (written out element by element from the index formulas), every
//    payload byte is written exactly once, and none comes from the staging buffer's poison;
//  * every run lies inside both sides, staging offsets are aligned, width_of divides what it is
//    used for;
//  * an unpacked problem equals the element-by-element copy out of that stride-7 handle: every
//    element where the map says, the zeroed tails zero, nothing else written;
//  * the rounds visit every entry exactly once; the header validates, and each tampering the
//    format promises to catch is caught.
// The arrays, their tags and the element-by-element copy are copy_map_hostcheck.cpp's.
#define main copy_map_hostcheck_main
#include "copy_map_hostcheck.cpp"
#undef main

#include "../../mhpc_minimal_env_amd/csrc/mhpc_snapshot_map.h"

namespace {
using mhpc_snap::payload_off;
using mhpc_snap::rec_bytes;
using mhpc_snap::stage_off;

struct Side {  // one side of a launch: array bases and extents in bytes
  char* base[A_N];
  size_t bytes[A_N];
};
template <class T>
Side side_of(Arrays<T>& a) {
  Side s;
  for (int i = 0; i < A_N; ++i) {
    s.base[i] = (char*)a.a[i].data();
    s.bytes[i] = a.a[i].size() * sizeof(T);
  }
  return s;
}
Side side_of(std::vector<unsigned char>& stage, const Dims& d, const Sizes& z, int R) {
  Side s;
  for (int i = 0; i < A_N; ++i) {
    s.base[i] = (char*)stage.data() + stage_off(d, z, i, R);
    s.bytes[i] = (size_t)R * rec_bytes(d, z, i);
  }
  return s;
}

// One pair of the launch: every block of the (run, chunk) table, as k_copy_problems does it.
void launch_pair(const char* what, const Side& s, const Side& d, const Dims& sd, const Dims& dd, const Sizes& z,
                 int bs, int bd, size_t chunk) {
  std::vector<int> table(block_table(sd, dd, z, chunk, nullptr));
  block_table(sd, dd, z, chunk, table.data());
  for (int e : table) {
    const Run q = run_of(sd, dd, z, bs, bd, e & 0xffff);
    const Piece p = piece_of(q, e >> 16, chunk);
    const size_t w = (size_t)width_of(q);
    CHECK(q.ncopy == 0 || q.so + q.ncopy <= s.bytes[q.arr], "%s: run %d reads past the source", what, e & 0xffff);
    CHECK(q.dof + q.ncopy + q.nzero <= d.bytes[q.arr], "%s: run %d writes past the destination", what, e & 0xffff);
    if ((q.ncopy && q.so + q.ncopy > s.bytes[q.arr]) || q.dof + q.ncopy + q.nzero > d.bytes[q.arr]) continue;
    CHECK(((uintptr_t)(s.base[q.arr] + q.so) % w == 0 || q.ncopy == 0) && (uintptr_t)(d.base[q.arr] + q.dof) % w == 0,
          "%s: run %d misaligned for width %zu", what, e & 0xffff, w);
    CHECK(p.c0 % w == 0 && (p.c1 - p.c0) % w == 0 && (p.z1 - p.c1) % w == 0, "%s: piece not a multiple of the width", what);
    if (p.c1 > p.c0) memcpy(d.base[q.arr] + q.dof + p.c0, s.base[q.arr] + q.so + p.c0, p.c1 - p.c0);
    if (p.z1 > p.c1) memset(d.base[q.arr] + q.dof + p.c1, 0, p.z1 - p.c1);
  }
}

// snap_move: `count` consecutive entries between the payload (n entries) and the staging records
void move(std::vector<unsigned char>& stage, std::vector<unsigned char>& payload, std::vector<unsigned char>* hits,
          const Dims& d, const Sizes& z, int R, int n, int entry, int slot, int count, bool to_host) {
  for (int a = 0; a < A_N; ++a) {
    const size_t rec = rec_bytes(d, z, a);
    if (rec == 0) continue;
    unsigned char* dev = stage.data() + stage_off(d, z, a, R) + (size_t)slot * rec;
    unsigned char* host = payload.data() + payload_off(d, z, a, n) + (size_t)entry * rec;
    if (to_host) {
      memcpy(host, dev, count * rec);
      for (size_t i = 0; hits && i < count * rec; ++i) ++(*hits)[host - payload.data() + i];
    } else {
      memcpy(dev, host, count * rec);
    }
  }
}

template <class T>
void snapshot_case(const char* what, int NKs, Dims store_s, int NKd, Dims store_d, size_t chunk) {
  const int nslot = 4, n = 8, R = 3, Bs = 9, NKb = 7;
  const int list[n] = {4, 0, 7, 2, 8, 1, 5, 3};
  const Dims sd{NKs, nslot, store_s.nbk, store_s.spmax};
  const Dims bd{NKb, nslot, store_s.nbk, store_s.spmax};  // the payload: the source's store shape, or none
  const Dims dd{NKd, nslot, store_d.nbk, store_d.spmax};
  const Sizes z = {(int)sizeof(T), (int)(ST_ELEMS * sizeof(T)), (int)(CARRY_ELEMS * sizeof(T))};
  const T dst_side = (T)1 << (8 * sizeof(T) - 1);
  Arrays<T> src(sd, Bs, 0);
  // the handle of stride 7 that holds the listed problems in list order: what the payload must be
  Arrays<T> mini(bd, n, dst_side);
  for (int i = 0; i < n; ++i) expect_copy(src, mini, sd, bd, list[i], i);
  size_t total = 0;
  for (int a = 0; a < A_N; ++a) {
    CHECK(rec_bytes(bd, z, a) * n == mini.a[a].size() * sizeof(T), "%s: rec_bytes of array %d", what, a);
    CHECK(payload_off(bd, z, a, n) == total, "%s: payload_off of array %d", what, a);
    CHECK(stage_off(bd, z, a, R) % mhpc_snap::STAGE_ALIGN == 0, "%s: staging base of array %d", what, a);
    total += rec_bytes(bd, z, a) * n;
  }
  CHECK(total == mhpc_snap::entry_payload_bytes(bd, z) * n, "%s: payload bytes per entry", what);
  // ---- pack, in rounds ----
  std::vector<unsigned char> payload(total, 0xCD), hits(total, 0);
  std::vector<int> seen(n, 0);
  CHECK(mhpc_snap::n_rounds(n, R) == 3, "%s: rounds", what);
  for (int r = 0; r < mhpc_snap::n_rounds(n, R); ++r) {
    int e0, cnt;
    mhpc_snap::round_of(n, R, r, &e0, &cnt);
    CHECK(cnt == (r < 2 ? 3 : 2) && e0 == 3 * r, "%s: round %d is [%d, +%d)", what, r, e0, cnt);
    std::vector<unsigned char> stage(mhpc_snap::stage_bytes(bd, z, R), 0xAB);
    const Side ss = side_of(src), st = side_of(stage, bd, z, R);
    for (int i = e0; i < e0 + cnt; ++i) {
      ++seen[i];
      launch_pair(what, ss, st, sd, bd, z, list[i], i % R, chunk);
    }
    move(stage, payload, &hits, bd, z, R, n, e0, 0, cnt, true);
  }
  for (int i = 0; i < n; ++i) CHECK(seen[i] == 1, "%s: entry %d visited %d times", what, i, seen[i]);
  for (size_t i = 0; i < total; ++i) CHECK(hits[i] == 1, "%s: payload byte %zu written %d times", what, i, hits[i]);
  for (int a = 0; a < A_N; ++a)
    CHECK(mini.a[a].empty() ||
              memcmp(payload.data() + payload_off(bd, z, a, n), mini.a[a].data(), mini.a[a].size() * sizeof(T)) == 0,
          "%s: payload of array %d", what, a);
  // ---- unpack entries (5, 2, 5, 7) into problems (1, 3, 0, 2) of a handle of 4, in rounds of distinct entries ----
  const int m = 4, Bd = 4, ent[m] = {5, 2, 5, 7}, dp[m] = {1, 3, 0, 2};
  Arrays<T> want(dd, Bd, dst_side), got(dd, Bd, dst_side);
  for (int i = 0; i < m; ++i) expect_copy(mini, want, bd, dd, ent[i], dp[i]);
  std::vector<int> uniq(ent, ent + m);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  const int Ru = 2;
  for (int r = 0; r < mhpc_snap::n_rounds((int)uniq.size(), Ru); ++r) {
    int u0, cnt;
    mhpc_snap::round_of((int)uniq.size(), Ru, r, &u0, &cnt);
    std::vector<unsigned char> stage(mhpc_snap::stage_bytes(bd, z, Ru), 0xAB);
    for (int a = 0; a < cnt; ++a) move(stage, payload, nullptr, bd, z, Ru, n, uniq[u0 + a], a, 1, false);
    const Side st = side_of(stage, bd, z, Ru), ds = side_of(got);
    for (int i = 0; i < m; ++i) {
      const int u = (int)(std::lower_bound(uniq.begin(), uniq.end(), ent[i]) - uniq.begin());
      if (u / Ru == r) launch_pair(what, st, ds, bd, dd, z, u % Ru, dp[i], chunk);
    }
  }
  for (int a = 0; a < A_N; ++a)
    for (size_t j = 0; j < got.a[a].size(); ++j)
      CHECK(got.a[a][j] == want.a[a][j], "%s: unpacked array %d element %zu", what, a, j);
}

void header_cases() {
  using namespace mhpc_snap;
  const Dims d{7, 4, 9, 5};
  const Sizes z{8, 37 * 8, 53 * 8};
  const uint32_t n = 3, eb = 40;
  Header h;
  memset(&h, 0, sizeof h);
  h.magic = MAGIC;
  h.version = FORMAT_VERSION;
  h.header_bytes = sizeof h;
  h.n_entries = n;
  h.entry_bytes = eb;
  h.precision = 64;
  h.elem_bytes = 8;
  h.sizeof_state = z.st;
  h.sizeof_carry = z.carry;
  h.nslot = d.nslot;
  h.NK = d.NK;
  h.nbk = d.nbk;
  h.spmax = d.spmax;
  h.payload_entry_bytes = entry_payload_bytes(d, z);
  h.total_bytes = sizeof h + (size_t)n * (eb + h.payload_entry_bytes);
  std::vector<unsigned char> blob(h.total_bytes, 0x5A);
  h.checksum = checksum_of(h, blob.data() + sizeof h);
  memcpy(blob.data(), &h, sizeof h);
  Header out;
  CHECK(validate(blob.data(), blob.size(), &out) == nullptr && out.n_entries == n && consistent(out) == nullptr,
        "a sound blob validates");
  out.sizeof_state += 8;
  CHECK(consistent(out) != nullptr, "a header whose sizes do not give its payload is inconsistent");
  auto refused = [&](const char* what, size_t off, size_t len, const char* word) {
    std::vector<unsigned char> b(blob);
    if (off < b.size()) b[off] ^= 1;
    const char* why = validate(b.data(), len, nullptr);
    CHECK(why && strstr(why, word), "%s: %s", what, why ? why : "accepted");
  };
  refused("short", blob.size(), 100, "shorter");
  refused("truncated", blob.size(), blob.size() - 1, "length");
  refused("magic", 0, blob.size(), "magic");
  refused("version", 8, blob.size(), "version");
  refused("entry table", sizeof h + 5, blob.size(), "checksum");
  refused("header field", 88, blob.size(), "checksum");  // alpha_bits
  blob[sizeof h + n * eb + 7] ^= 1;  // the payload is not covered: it is the caller's data
  CHECK(validate(blob.data(), blob.size(), nullptr) == nullptr, "payload bytes are not part of the checksum");
  CHECK(default_round(100, 1000, 50) == 10 && default_round(100, 50, 5) == 1 && default_round(100, 1000, 4) == 4,
        "default_round");
}

template <class T>
void snapshot_cases() {
  const Dims none{0, 0, 0, 0}, a{0, 0, 9, 5}, b{0, 0, 11, 4};
  char what[96];
  for (int NKs : {12, 7})
    for (int NKd : {7, 12})
      for (const Dims* ss : {&a, &none})
        for (const Dims* ds : {&a, &b, &none})
          for (size_t chunk : {(size_t)48, (size_t)16384}) {
            snprintf(what, sizeof what, "%zu-byte NK %d->7->%d store (%d,%d)->(%d,%d) chunk %zu", sizeof(T), NKs,
                     NKd, ss->nbk, ss->spmax, ds->nbk, ds->spmax, chunk);
            snapshot_case<T>(what, NKs, *ss, NKd, *ds, chunk);
          }
}
}  // namespace

int main() {
  snapshot_cases<uint64_t>();
  snapshot_cases<uint32_t>();
  header_cases();
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
