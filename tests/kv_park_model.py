"""The blob of a parked sequence (zgml_amd/csrc/kv_park.h) restated in numpy, shared by tests/test_kv_park_host.py (the header
against this model) and tests/test_hip_kv_park.py (the device's blobs against this model, byte for byte).

A lane is described as the C ABI describes it — (buf, offset, d_head, n_cols, block_size) — and its parked columns are handed over as
arrays: f32 [n, d_head] for an f32 lane, (int8 [n, d_head], f32 scales [n, d_head / 32]) for an int8 lane. The bytes between a
run's end and the next 16-byte boundary are zero."""
import numpy as np

from tests.kv_shift_model import quantise

f32 = np.float32
MAGIC, VERSION, INT8 = 0x50564B5A, 1, 1
HEADER, RECORD = 32, 16
F32, I8 = 0, 1

HEADER_DT = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_lanes", "<u8"), ("n", "<u4"), ("flags", "<u4"), ("total", "<u8")])
RECORD_DT = np.dtype([("d_head", "<u4"), ("form", "<u4"), ("offset", "<u8")])
LANE_DT = np.dtype([("buf", "<u2"), ("_pad", "<u2"), ("d_head", "<u4"), ("n_cols", "<u4"), ("block_size", "<u4"), ("offset", "<u8")])  # zgml_kv_lane
assert HEADER_DT.itemsize == HEADER and RECORD_DT.itemsize == RECORD and LANE_DT.itemsize == 24


def align16(x):
    return (x + 15) & ~15


def lane_table(lanes):
    """[(buf, offset, d_head, n_cols, block_size)] -> the zgml_kv_lane array as bytes"""
    t = np.zeros(len(lanes), LANE_DT)
    for i, (buf, off, dh, nc, bs) in enumerate(lanes):
        t[i] = (buf, 0, dh, nc, bs, off)
    return t


def form(block_size, flags):
    return I8 if block_size or flags & INT8 else F32


def layout(lanes, n, flags=0):
    """-> (total bytes, [(d_head, form, data offset, scales offset or None)]); lanes: [(buf, offset, d_head, n_cols, block_size)]"""
    if n == 0 or not lanes:
        return HEADER, []
    off, recs = HEADER + RECORD * len(lanes), []
    for _, _, dh, _, bs in lanes:
        fm = form(bs, flags)
        if fm == I8:
            sc = align16(off + n * dh)
            recs.append((dh, fm, off, sc))
            off = align16(sc + n * dh // 32 * 4)
        else:
            recs.append((dh, fm, off, None))
            off = align16(off + n * dh * 4)
    return off, recs


def head(lanes, n, flags=0):
    """the bytes the HOST writes: header and directory"""
    total, recs = layout(lanes, n, flags)
    h = np.zeros(1, HEADER_DT)
    h[0] = (MAGIC, VERSION, len(recs), n if recs else 0, flags, total)
    d = np.zeros(len(recs), RECORD_DT)
    for i, (dh, fm, off, _) in enumerate(recs):
        d[i] = (dh, fm, off)
    return np.concatenate([h.view(np.uint8), d.view(np.uint8)])


def blob(lanes, cols, n, flags=0):
    """The whole blob. cols[i]: lane i's parked columns — f32 [n, d_head], or (int8 [n, d_head], scales [n, d_head / 32]) for an int8
    lane. An f32 lane under INT8 is quantised with the column rule (tests/kv_shift_model.quantise). -> uint8 blob"""
    total, recs = layout(lanes, n, flags)
    out = np.zeros(total, np.uint8)
    hd = head(lanes, n, flags)
    out[:hd.size] = hd
    for (_, _, dh, _, bs), c, (_, fm, off, sc) in zip(lanes, cols, recs):
        if fm == F32:
            run = np.ascontiguousarray(c, f32).reshape(n * dh).view(np.uint8)
            out[off:off + run.size] = run
            continue
        q, s = c if bs else quantise(np.asarray(c, f32).reshape(n, dh))
        q, s = np.ascontiguousarray(q, np.int8).reshape(n * dh).view(np.uint8), np.ascontiguousarray(s, f32).reshape(n * dh // 32).view(np.uint8)
        out[off:off + q.size] = q
        out[sc:sc + s.size] = s
    return out
