// The snapshot blob of mhpc_snapshot_problems / mhpc_restore_problems and the staging side of its
// device path, as plain arithmetic on top of mhpc_copy_map.h.
//
// A snapshot is the mhpc_copy_problems of the listed problems into a handle that exists only as
// bytes: a "staging side" with Dims of its own (knot stride NK = the longest listed layout, the
// source's slot count and store shape, a batch of R problems -- one round) whose arrays lie one
// behind the other in one device buffer.  Pack is run_of(source handle -> staging), unpack is
// run_of(staging -> destination handle): the same map, the same kernel (k_copy_problems) and the
// same host check (tests/native/snapshot_map_hostcheck.cpp) in both directions.  Nothing here
// depends on array contents.
//
// Blob = Header | entry table [n][entry_bytes] | payload.  The payload is array-major: for each
// array of mhpc_copy::Arr in turn the records of entries 0..n-1, each rec_bytes() long, so entry e
// of array a lies at payload_off(a, n) + e * rec_bytes(a) whatever the round size was, and a
// round of consecutive entries moves between host and device with one copy per array.  The
// staging buffer holds the same records with every array's base aligned to STAGE_ALIGN (the
// alignment bytes are never copied to the blob).
#pragma once
#include <stdint.h>
#include <string.h>

#include "mhpc_copy_map.h"

namespace mhpc_snap {

using mhpc_copy::Dims;
using mhpc_copy::Sizes;

constexpr uint64_t MAGIC = 0x3150414e5343484dull;  // "MHCSNAP1", little endian
// Bumped by any change to ProbState, BwsCarry, the record widths below, the entry record or this
// header: a blob is only ever read by the format that wrote it.
constexpr uint32_t FORMAT_VERSION = 1;
constexpr size_t STAGE_ALIGN = 256;

struct Header {  // 128 bytes, fixed-width fields, no padding
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t checksum;  // fnv1a (below) of the header (this field zero), then the entry table
  uint32_t n_entries, entry_bytes;
  uint32_t precision, elem_bytes;
  uint32_t sizeof_state, sizeof_carry;
  uint32_t KS, PS, PS_JAC, SREC, MAXP, nslot;
  uint64_t alpha_bits;
  uint32_t sweep32, x0_row;
  uint32_t NK, nbk, spmax;  // the payload's Dims (with nslot)
  uint32_t need_full, solved, reserved;
  uint64_t payload_entry_bytes;
};
static_assert(sizeof(Header) == 128, "the header is part of the format");

// Bytes of one problem's record of array a under dims d: the extent run_of covers there.
inline size_t rec_bytes(const Dims& d, const Sizes& z, int a) {
  using namespace mhpc_copy;
  const size_t E = (size_t)z.real, NK = (size_t)d.NK;
  switch (a) {
    case A_TRAJ: return (size_t)d.nslot * NK * KS * E;
    case A_PAR: return NK * PS * E;
    case A_REFPOS: return NK * E;
    case A_K: return NK * 56 * E;
    case A_DU: return NK * 4 * E;
    case A_G: return NK * 14 * E;
    case A_PX: return (size_t)MAXP * 196 * E;
    case A_X0: return 14 * E;
    case A_ST: return (size_t)z.st;
    case A_CARRY: return (size_t)z.carry;
    case A_CMD: return 2 * E;
    default: return (size_t)d.spmax * d.nbk * SREC * E;
  }
}
inline size_t entry_payload_bytes(const Dims& d, const Sizes& z) {
  size_t s = 0;
  for (int a = 0; a < mhpc_copy::A_N; ++a) s += rec_bytes(d, z, a);
  return s;
}
// Offset of array a's records in the payload of a blob of n entries.
inline size_t payload_off(const Dims& d, const Sizes& z, int a, size_t n) {
  size_t s = 0;
  for (int i = 0; i < a; ++i) s += n * rec_bytes(d, z, i);
  return s;
}
// Offset of array a's base in a staging buffer of R problems, and the buffer's size.
inline size_t stage_off(const Dims& d, const Sizes& z, int a, size_t R) {
  size_t s = 0;
  for (int i = 0; i < a; ++i) s += (R * rec_bytes(d, z, i) + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN;
  return s;
}
inline size_t stage_bytes(const Dims& d, const Sizes& z, size_t R) {
  return stage_off(d, z, mhpc_copy::A_N, R);
}

// Rounds of R entries over n: round r covers [first, first + count).
inline int n_rounds(int n, int R) { return (n + R - 1) / R; }
inline void round_of(int n, int R, int r, int* first, int* count) {
  *first = r * R;
  *count = n - *first < R ? n - *first : R;
}
// The default round: as many problems as fit `cap` bytes of staging, at least one, at most n.
inline int default_round(size_t entry_bytes, size_t cap, int n) {
  size_t R = entry_bytes ? cap / entry_bytes : (size_t)n;
  if (R < 1) R = 1;
  return R > (size_t)n ? n : (int)R;
}

// FNV-1a 64 taken over little-endian 64-bit words (header and entry records are multiples of 8
// bytes; a shorter tail would be zero-extended): every reader checks the whole entry table, so
// the checksum is eight times cheaper than the byte-wise one.
inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i += 8) {
    uint64_t w = 0;
    memcpy(&w, b + i, n - i < 8 ? n - i : 8);
    h = (h ^ w) * 0x100000001b3ull;
  }
  return h;
}
inline uint64_t checksum_of(const Header& h, const void* entries) {
  Header c = h;
  c.checksum = 0;
  return fnv1a(entries, (size_t)h.n_entries * h.entry_bytes, fnv1a(&c, sizeof c));
}

inline Dims dims_of(const Header& h) {
  return Dims{(int)h.NK, (int)h.nslot, (int)h.nbk, (int)h.spmax};
}
inline Sizes sizes_of(const Header& h) {
  return Sizes{(int)h.elem_bytes, (int)h.sizeof_state, (int)h.sizeof_carry};
}

// What every reader checks before it believes a blob, in this order; null: the blob is sound
// (precision-independent: the build's own sizes are compared by the instantiation that reads it).
inline const char* validate(const void* blob, size_t bytes, Header* out) {
  if (!blob || bytes < sizeof(Header)) return "snapshot blob shorter than its header";
  Header h;
  memcpy(&h, blob, sizeof h);
  if (h.magic != MAGIC) return "not a snapshot blob (wrong magic)";
  if (h.version != FORMAT_VERSION) return "snapshot of another format version";
  if (h.header_bytes != sizeof(Header) || h.n_entries < 1 || h.entry_bytes > (1u << 20) ||
      h.NK < 1 || h.NK > 65536 || h.nslot < 1 || h.nslot > 64 || h.nbk > 65536 || h.spmax > 64 ||
      h.elem_bytes > 8 || h.sizeof_state > (1u << 20) || h.sizeof_carry > (1u << 20))
    return "snapshot header out of range";
  const size_t table = (size_t)h.n_entries * h.entry_bytes;
  if (h.payload_entry_bytes > ((uint64_t)1 << 40)) return "snapshot header out of range";
  if (h.total_bytes != sizeof(Header) + table + (size_t)h.n_entries * h.payload_entry_bytes)
    return "snapshot header inconsistent (total length)";
  if (bytes != h.total_bytes) return "snapshot length does not match its header (truncated?)";
  if (checksum_of(h, (const char*)blob + sizeof h) != h.checksum)
    return "snapshot header / entry table checksum mismatch";
  if (out) *out = h;
  return nullptr;
}
// ... and, once a reader knows the header's sizes are its own build's (or has none to compare):
// the payload's extent follows from the header's dimensions.
inline const char* consistent(const Header& h) {
  return h.payload_entry_bytes == entry_payload_bytes(dims_of(h), sizes_of(h))
             ? nullptr
             : "snapshot header inconsistent (payload bytes per entry)";
}

}  // namespace mhpc_snap
