"""Snapshot blobs on the host: mhpc_snapshot_info / mhpc_snapshot_entry / mhpc_snapshot_status need
no handle and no GPU.  They read the committed golden blob (tests/golden/snapshot_v1.bin, written
by tests/golden/make_snapshot_golden.py), refuse every tampering the format promises to catch, and
the ctypes mirror of the new struct has the header's size."""
import ctypes
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER_BYTES, OFF_VERSION, OFF_CHECKSUM, OFF_ENTRIES, OFF_STATE = 128, 8, 24, 32, 48


@pytest.fixture(scope="module")
def blob():
    from mhpc_minimal_env_amd import capi, locomotion as L
    if not os.path.exists(capi.LIB_PATH):
        pytest.fail("libmhpc_amd.so not built (run __graft_entry__.build())")
    return L.load_snapshot(os.path.join(GOLD, "snapshot_v1.bin"))


def _fnv1a(data, h=0xcbf29ce484222325):
    """FNV-1a 64 over little-endian 64-bit words (mhpc_snapshot_map.h)."""
    data = bytes(data)
    for (w,) in struct.iter_unpack("<Q", data + b"\0" * (-len(data) % 8)):
        h = ((h ^ w) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _resealed(b):
    b = bytearray(b.tobytes())
    n, eb = struct.unpack_from("<II", b, OFF_ENTRIES)
    struct.pack_into("<Q", b, OFF_CHECKSUM, 0)
    struct.pack_into("<Q", b, OFF_CHECKSUM, _fnv1a(b[HEADER_BYTES:HEADER_BYTES + n * eb], _fnv1a(b[:HEADER_BYTES])))
    return np.frombuffer(bytes(b), dtype=np.uint8)


def test_info_and_entry_of_the_golden_blob(blob):
    from mhpc_minimal_env_amd import capi, locomotion as L
    sys.path.insert(0, GOLD)
    from make_snapshot_golden import golden_desc
    want = json.load(open(os.path.join(GOLD, "snapshot_v1.json")))
    info = L.snapshot_info(blob)
    assert info["version"] == capi.MHPC_SNAPSHOT_VERSION == want["version"]
    assert info["total_bytes"] == blob.size == want["bytes"] <= 256 * 1024
    assert info["n_entries"] == 1 and info["precision"] == 64 and info["sweep_bits"] == 64
    assert info["x0_row"] == 14 and info["knot_stride"] == 16 and info["alpha"] == L.HSDDP_OPTION().alpha
    assert info["store_buffers"] == 0 and info["need_full"] == 0 and info["solved"] == 0
    assert blob.size == HEADER_BYTES + struct.unpack_from("<I", blob, OFF_ENTRIES + 4)[0] + info["payload_bytes_per_entry"]
    # the recomputed checksum is the stored one: the documented FNV-1a 64
    assert np.array_equal(_resealed(blob), blob)
    e = L.snapshot_entry(blob, 0)
    assert bytes(e["desc"]) == bytes(golden_desc())
    assert e["option"] == L.HSDDP_OPTION() and e["status"] == 0
    assert bytes(e["weights"]) == bytes(capi.default_cost_weights())
    assert bytes(e["constraints"]) == bytes(capi.default_constraint_params())


def test_validation_refusals(blob):
    from mhpc_minimal_env_amd import capi
    lib = capi.lib()

    def tampered(off, delta=1, reseal=False):
        b = blob.copy()
        b[off] = (int(b[off]) + delta) & 0xFF
        return _resealed(b) if reseal else b

    def calls(b, entry=0):
        info, d, st = capi.SnapshotInfo(), capi.ProblemDesc(), ctypes.c_int32(0)
        return (lib.mhpc_snapshot_info(b.ctypes.data, int(b.size), ctypes.byref(info)),
                lib.mhpc_snapshot_entry(b.ctypes.data, int(b.size), entry, ctypes.byref(d), None, None, None),
                lib.mhpc_snapshot_status(b.ctypes.data, int(b.size), entry, 1, ctypes.byref(st)))

    INV = capi.MHPC_ERR_INVALID
    assert calls(blob) == (0, 0, 0)
    for what, bad, word in (("truncated", blob[:-1].copy(), b"length"),
                            ("shorter than a header", blob[:64].copy(), b"shorter"),
                            ("longer than the header says", np.concatenate([blob, blob[:1]]), b"length"),
                            ("wrong magic", tampered(3), b"magic"),
                            ("bumped version", tampered(OFF_VERSION), b"version"),
                            ("flipped entry byte", tampered(HEADER_BYTES + 40), b"checksum"),
                            ("flipped header byte", tampered(90), b"checksum")):
        assert calls(bad) == (INV, INV, INV), what
        assert word in lib.mhpc_last_error(), (what, lib.mhpc_last_error())
    # a header whose build sizes differ, sealed again: its entries belong to another build (and the
    # header reader, which compares no build sizes, finds the payload's extent inconsistent)
    other = tampered(OFF_STATE, 8, reseal=True)
    rc = calls(other)
    assert rc == (INV, INV, INV) and b"ProbState" in lib.mhpc_last_error(), lib.mhpc_last_error()
    assert calls(blob, entry=1)[1:] == (INV, INV) and b"entry out of range" in lib.mhpc_last_error()
    assert calls(blob, entry=-1)[1:] == (INV, INV)
    assert lib.mhpc_snapshot_info(None, 0, ctypes.byref(capi.SnapshotInfo())) == INV
    assert lib.mhpc_snapshot_info(blob.ctypes.data, int(blob.size), None) == INV


def test_new_struct_layout_matches_header():
    """ctypes size of struct mhpc_snapshot_info against a compiled probe (C, as the header is)."""
    from mhpc_minimal_env_amd import capi
    src = ('#include "mhpc_capi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %d",'
           'sizeof(struct mhpc_snapshot_info),offsetof(struct mhpc_snapshot_info,alpha),'
           'offsetof(struct mhpc_snapshot_info,total_bytes),MHPC_SNAPSHOT_VERSION);}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "p")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(capi.SnapshotInfo), capi.SnapshotInfo.alpha.offset,
                                     capi.SnapshotInfo.total_bytes.offset, capi.MHPC_SNAPSHOT_VERSION]
