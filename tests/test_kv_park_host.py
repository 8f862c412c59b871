"""CPU tests of the parked blob's layout (zgml_amd/csrc/kv_park.h): the header, compiled alone for the CPU
(tests/cpp/kv_park_probe.cpp), against the numpy model of tests/kv_park_model.py — sizes, offsets and the bytes the host writes, on
lane tables that mix f32 and int8 lanes —; every refusal the header makes, with its text; and zgml_hip_kv_park_bytes of the built
library (it needs no GPU) on the same tables: the model's size, 0 for a refused table."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import kv_park_model as M
from zgml_amd import capi

ROOT = Path(__file__).resolve().parent.parent
PAD = 0xEE  # what the probe leaves where the device would write


def kv_park_probe():
    src, exe = ROOT / "tests" / "cpp" / "kv_park_probe.cpp", ROOT / "tests" / "cpp" / "_build" / "kv_park_probe"
    hdrs = [ROOT / "zgml_amd" / "csrc" / "kv_park.h", ROOT / "include" / "zgml_hip.h"]
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    return exe


def run(*args):
    return subprocess.run([str(kv_park_probe()), *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()


def table_file(tmp_path, lanes):
    if lanes is None:
        return "-"
    path = tmp_path / "lanes.bin"
    M.lane_table(lanes).tofile(path)
    return path


def probe_layout(tmp_path, lanes, n, flags=0, cap="-", n_lanes=None):
    """-> (kvp_park_bytes, total or None, refusal text or None, the host-written blob or None)"""
    out = tmp_path / "blob.bin"
    lines = run("layout", n, flags, table_file(tmp_path, lanes), len(lanes or []) if n_lanes is None else n_lanes, cap, out)
    size = int(lines[0].split()[1])
    if lines[1].startswith("refused: "):
        return size, None, lines[1][len("refused: "):], None
    return size, int(lines[1].split()[1]), None, np.fromfile(out, np.uint8)


def probe_check(tmp_path, blob, lanes, nbytes="-", n_lanes=None):
    """-> "ok <n> <n_lanes>" or the refusal text"""
    path = "-"
    if blob is not None:
        path = tmp_path / "in.bin"
        np.asarray(blob, np.uint8).tofile(path)
    line = run("check", path, nbytes, table_file(tmp_path, lanes), len(lanes or []) if n_lanes is None else n_lanes)[0]
    return line[len("refused: "):] if line.startswith("refused: ") else line


def lib_bytes(lanes, n, flags=0, n_lanes=None):
    t = M.lane_table(lanes or [])
    arr = (capi.KvLaneC * max(1, len(t))).from_buffer_copy(t.tobytes().ljust(24, b"\0"))
    return int(capi.load_hip().zgml_hip_kv_park_bytes(arr if lanes is not None else None, len(t) if n_lanes is None else n_lanes, n, flags))


# (buf, offset, d_head, n_cols, block_size): f32 lanes of d_head 8, 32, 64, 80 and 128 (one at an odd offset) between int8 lanes of
# 32, 64 and 128
MIXED = [(0, 0, 8, 300, 0), (1, 0, 32, 300, 32), (0, 2401, 32, 300, 0), (2, 0, 64, 300, 32), (3, 0, 64, 300, 0), (3, 19200, 80, 300, 0),
         (4, 0, 128, 300, 32), (5, 0, 128, 300, 0)]
F32_ONLY = [(0, 0, 8, 300, 0), (0, 2400, 80, 300, 0), (1, 0, 128, 300, 0)]
I8_ONLY = [(1, 0, 32, 300, 32), (2, 0, 128, 300, 32)]
INT8_ABLE = [l for l in MIXED if l[2] % 32 == 0]


@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("name,lanes,flags", [("mixed", MIXED, 0), ("f32", F32_ONLY, 0), ("int8", I8_ONLY, 0), ("int8 flag", INT8_ABLE, M.INT8),
                                               ("int8 flag on int8 lanes", I8_ONLY, M.INT8), ("one lane", MIXED[:1], 0)])
def test_size_offsets_and_host_bytes_equal_the_model(tmp_path, name, lanes, flags, n):
    total, recs = M.layout(lanes, n, flags)
    size, got_total, why, blob = probe_layout(tmp_path, lanes, n, flags)
    assert why is None and size == got_total == total == blob.size, (why, size, got_total, total)
    assert lib_bytes(lanes, n, flags) == total
    # every run on a 16-byte boundary, in lane order, none beyond the total; an int8 run of an f32 lane only under the flag
    end = M.HEADER + M.RECORD * len(lanes)
    for (_, _, dh, _, bs), (rdh, fm, off, sc) in zip(lanes, recs):
        assert rdh == dh and fm == (M.I8 if bs or flags & M.INT8 else M.F32)
        assert off % 16 == 0 and off == end
        end = M.align16(off + n * dh * 4) if fm == M.F32 else M.align16(M.align16(off + n * dh) + n * dh // 32 * 4)
        assert sc is None or (sc % 16 == 0 and sc == M.align16(off + n * dh))
    assert end == total
    # the host's bytes: header and directory are the model's; the model's blob over all-0xEE columns is the probe's blob, gaps included
    hd = M.head(lanes, n, flags)
    assert np.array_equal(blob[:hd.size], hd)
    cols = []
    for (_, _, dh, _, bs), (_, fm, _, _) in zip(lanes, recs):
        cols.append((np.full((n, dh), PAD, np.uint8).view(np.int8), np.full((n, dh // 8), PAD, np.uint8).view(np.float32)) if fm == M.I8
                    else np.full((n, dh * 4), PAD, np.uint8).view(np.float32))
    as_int8 = [(b, o, dh, nc, 32 if fm == M.I8 else 0) for (b, o, dh, nc, _), (_, fm, _, _) in zip(lanes, recs)]  # (runs handed over ready-made)
    want = M.blob(as_int8, cols, n)
    want[:hd.size] = hd
    assert np.array_equal(blob, want)
    # and the blob passes the resume's check against its own table (and an int8 destination for every lane)
    assert probe_check(tmp_path, blob, lanes if not flags else as_int8) == f"ok {n} {len(lanes)}"


def test_the_int8_flag_shrinks_f32_lanes_to_the_documented_share():
    lanes = [(0, 0, 128, 2048, 0)] * 4
    plain, small = M.layout(lanes, 2048)[0], M.layout(lanes, 2048, M.INT8)[0]
    assert lib_bytes(lanes, 2048) == plain and lib_bytes(lanes, 2048, M.INT8) == small
    assert abs(small / plain - (1 + 4 / 32) / 4) < 1e-3  # a byte and 1/32 of a float per value against a float: 0.28


def test_empty_blobs(tmp_path):
    for lanes, n, n_lanes in [(MIXED, 0, None), ([], 5, None), (None, 5, 0), ([(9, 3, 0, 0, 7)], 0, None)]:
        size, total, why, blob = probe_layout(tmp_path, lanes, n, 0, n_lanes=n_lanes)
        assert why is None and size == total == M.HEADER
        assert np.array_equal(blob, M.head([], 0))
        assert lib_bytes(lanes, n, 0, n_lanes) == M.HEADER
        assert probe_check(tmp_path, blob, MIXED) == "ok 0 0"  # (an empty blob resumes into anything: nothing happens)


PARK_REFUSALS = [  # (word, lanes, n, flags, cap, n_lanes)
    ("block_size", [(0, 0, 64, 16, 16)], 4, 0, "-", None),
    ("must not be 0", [(0, 0, 0, 16, 0)], 4, 0, "-", None),
    ("must not be 0", [(0, 0, 64, 0, 0)], 4, 0, "-", None),
    ("n_cols", [(0, 0, 64, 16, 0), (0, 0, 64, 3, 0)], 4, 0, "-", None),
    ("d_head % 32", [(1, 0, 48, 16, 32)], 4, 0, "-", None),
    ("offset", [(1, 4, 64, 16, 32)], 4, 0, "-", None),
    ("KV_PARK_INT8", [(0, 0, 64, 16, 0), (0, 0, 80, 16, 0)], 4, M.INT8, "-", None),
    ("KV_PARK_INT8", [(0, 0, 8, 16, 0)], 4, M.INT8, "-", None),
    ("flags", [(0, 0, 64, 16, 0)], 4, 2, "-", None),
    ("lane records", None, 4, 0, "-", 3),
]


@pytest.mark.parametrize("word,lanes,n,flags,cap,n_lanes", PARK_REFUSALS)
def test_park_refusals_by_the_records_alone(tmp_path, word, lanes, n, flags, cap, n_lanes):
    size, total, why, _ = probe_layout(tmp_path, lanes, n, flags, cap, n_lanes)
    assert size == 0 and total is None and word in why, (word, why)
    assert lib_bytes(lanes, n, flags, n_lanes) == 0
    if lanes and len(lanes) > 1:
        assert why.startswith("lane 1: ")  # (the lane at fault is named)


def test_park_refuses_a_cap_below_the_size(tmp_path):
    total = M.layout(MIXED, 3)[0]
    size, got, why, _ = probe_layout(tmp_path, MIXED, 3, 0, total - 1)
    assert size == total and got is None and "cap below" in why
    assert probe_layout(tmp_path, MIXED, 3, 0, total + 5)[1] == total  # (more room than needed is fine)
    assert "cap below" in probe_layout(tmp_path, MIXED, 0, 0, M.HEADER - 1)[2]  # (an empty blob needs its header's room)


def good_blob(lanes, n, flags=0):
    total, _ = M.layout(lanes, n, flags)
    blob = np.zeros(total, np.uint8)
    hd = M.head(lanes, n, flags)
    blob[:hd.size] = hd
    return blob


def patched(blob, dt, index, field, value, base=0):
    out = blob.copy()
    rec = out[base + index * dt.itemsize:base + (index + 1) * dt.itemsize].view(dt)
    rec[field] = value
    return out


def test_resume_refusals_by_the_blob_and_the_records(tmp_path):
    lanes = [(0, 0, 64, 16, 0), (1, 0, 64, 16, 32), (0, 1024, 8, 16, 0)]
    blob = good_blob(lanes, 3)
    all_i8 = [(0, 0, 64, 16, 32), (1, 0, 64, 16, 32)]
    cases = [
        ("no blob", None, lanes, "-"),
        ("below a header", blob[:31], lanes, "-"),
        ("magic", patched(blob, M.HEADER_DT, 0, "magic", M.MAGIC + 1), lanes, "-"),
        ("version", patched(blob, M.HEADER_DT, 0, "version", 2), lanes, "-"),
        ("differ from the header's total", blob, lanes, blob.size - 16),        # a truncated blob
        ("differ from the header's total", np.concatenate([blob, blob[:16]]), lanes, "-"),
        ("flags", patched(blob, M.HEADER_DT, 0, "flags", 4), lanes, "-"),
        ("n_lanes differs", blob, lanes[:2], "-"),
        ("n_lanes differs", blob, lanes + lanes[:1], "-"),
        ("d_head differs", blob, [lanes[0], lanes[1], (0, 1024, 16, 16, 0)], "-"),
        ("int8 -> f32", blob, [lanes[0], (0, 2048, 64, 16, 0), lanes[2]], "-"),
        ("int8 -> f32", good_blob(all_i8[:1], 3, M.INT8), [(0, 0, 64, 16, 0)], "-"),  # (parked quantised from an f32 lane)
        ("form", patched(blob, M.RECORD_DT, 1, "form", 2, M.HEADER), lanes, "-"),
        ("not the layout's", patched(blob, M.RECORD_DT, 1, "offset", 4096, M.HEADER), lanes, "-"),  # a directory that points elsewhere
        ("not the layout's", patched(blob, M.HEADER_DT, 0, "n", 4), lanes, "-"),                     # more columns than the total holds
        ("lane records", blob, None, "-"),
        ("empty blob", patched(blob, M.HEADER_DT, 0, "n", 0), lanes, "-"),
    ]
    for word, b, table, nbytes in cases:
        n_lanes = 3 if table is None else None
        got = probe_check(tmp_path, b, table, nbytes, n_lanes)
        assert not got.startswith("ok") and word in got, (word, got)
    # what is allowed: the same blob into lanes of other n_cols / offsets / buffers, f32 runs into int8 lanes
    assert probe_check(tmp_path, blob, [(7, 64, 64, 99, 0), (2, 0, 64, 5, 32), (3, 1, 8, 3, 0)]) == "ok 3 3"
    assert probe_check(tmp_path, good_blob(lanes[:2], 3), all_i8) == "ok 3 2"


def test_the_wrappers_are_hip_only(oracle):
    """Session.park / resume and BatchSession.park / resume on an oracle session: a RuntimeError that says a HIP session is needed
    (like admit / fork / shift), before anything else is looked at."""
    from zgml_amd import llama
    m = llama.Model(llama.preset("tiny"))
    s = llama.Session(m, oracle.backend_fns())
    with pytest.raises(RuntimeError, match="HIP session"):
        s.park(4)
    with pytest.raises(RuntimeError, match="HIP session"):
        s.resume(np.zeros(32, np.uint8))
    bs = llama.BatchSession(m, oracle.backend_fns(), 2)
    with pytest.raises(RuntimeError, match="HIP session"):
        bs.park(1, 4)
    with pytest.raises(RuntimeError, match="HIP session"):
        bs.resume(1, np.zeros(32, np.uint8))
    bs.close(), s.close(), m.close()
