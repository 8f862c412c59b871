"""Properties of the dependency schedule (zgml_amd/csrc/schedule.hip) on the CPU: the access spans it declares per op, the
overlap test between spans, the levels it puts ops on, and the bounds it assumes for dynamic fields. Everything the launch
planner fuses or reorders rests on these; a footprint missing here is a race on the GPU. The shim tests/cpp/schedule_probe.cpp
is built with g++ against schedule.hip compiled as plain C++; the oracle (oracle/zgml_oracle.c) runs the ops."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd.program import ops_to_c
from tests import plan_cases as PC

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "cpp" / "_build" / "libschedule_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "schedule_probe.cpp", ROOT / "zgml_amd" / "csrc" / "schedule.hip",
        ROOT / "zgml_amd" / "csrc" / "schedule.h", ROOT / "include" / "zgml_hip.h"]
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", str(ROOT / "include"), "-o", str(LIB),
                        str(SRCS[0]), "-x", "c++", str(SRCS[1])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u64 = C.c_void_p, C.c_uint64
    lib.zs_schedule.argtypes = [vp, u64, vp, u64, vp, u64, vp, vp, vp, vp, u64, vp]
    lib.zs_schedule.restype = C.c_int
    lib.zs_overlap_matrix.argtypes, lib.zs_overlap_matrix.restype = [vp, u64, vp], None
    lib.zs_dynamic_field_in_bounds.argtypes, lib.zs_dynamic_field_in_bounds.restype = [vp, u64, vp, u64, vp, vp, vp], None
    lib.zs_dyn_field.argtypes, lib.zs_dyn_field.restype = [vp, C.c_uint32, vp], None
    _lib = lib
    return lib


def schedule(ops, sizes, barriers=(), seq_kv_bound=None, refreshed=None):
    """-> (levels, spans: rows of (op, is_write, buf, lo, hi, period, width), dynamic_fields_in_bounds(refreshed) or None)"""
    lib = probe()
    arr, keep = ops_to_c(ops)
    ref = ops_to_c(refreshed) if refreshed is not None else None
    n = len(ops)
    sz = np.array(sizes, np.uint64)
    bar = np.array(list(barriers) or [0], np.uint64)
    bound = np.array(seq_kv_bound, np.uint32) if seq_kv_bound is not None else None
    level = np.zeros(n, np.uint32)
    cap = 16 * n + 16
    spans = np.zeros((cap, 7), np.uint64)
    n_spans = C.c_uint64()
    r = lib.zs_schedule(C.addressof(arr), n, sz.ctypes.data, len(sizes), bar.ctypes.data, len(barriers),
                        bound.ctypes.data if bound is not None else None, C.addressof(ref[0]) if ref else None,
                        level.ctypes.data, spans.ctypes.data, cap, C.byref(n_spans))
    assert n_spans.value <= cap
    return level, spans[:n_spans.value], (None if r < 0 else bool(r))


def span_mask(span, size):
    """the elements of one declared span as a boolean mask over a buffer of `size` elements"""
    lo, hi, period, width = (int(v) for v in span[3:7])
    m = np.zeros(size, bool)
    if period == 0:
        m[lo:min(hi, size)] = True
    else:
        for start in range(lo, hi, period):
            m[start:min(start + width, hi, size)] = True
    return m


def footprint(spans, op, write, buf, size):
    m = np.zeros(size, bool)
    for s in spans:
        if int(s[0]) == op and (write is None or int(s[1]) == write) and int(s[2]) == buf:
            m |= span_mask(s, size)
    return m


# ── 1. spans_overlap against element sets ──────────────────────────────────────────────────────────────────────────────

def _all_spans():
    """dense intervals and periodic runs (both residue orders, runs that wrap the period, width == period) over [0, 24)"""
    out = []
    for lo in range(0, 9):
        for n in (1, 2, 5, 9):
            out.append((0, lo, lo + n, 0, 0))
        for P in (2, 3, 4, 5):
            for W in range(1, P + 1):
                for runs in (1, 2, 3):
                    out.append((0, lo, lo + (runs - 1) * P + W, P, W))
    return out


def test_spans_overlap_never_misses_a_shared_element():
    rows = _all_spans()
    n = len(rows)
    got = np.zeros((n, n), np.uint8)
    arr = np.array(rows, np.uint64)
    probe().zs_overlap_matrix(arr.ctypes.data, n, got.ctypes.data)
    elems = np.stack([span_mask(np.array((0, 0) + r, np.uint64), 32) for r in rows]).astype(np.int32)
    meet = (elems @ elems.T) > 0
    missed = np.argwhere(meet & (got == 0))
    assert missed.size == 0, [(rows[i], rows[j]) for i, j in missed[:5]]
    # and the periodic form does separate disjoint residues (otherwise it would be pointless): P = 4, runs at 0 and 2
    a, b = rows.index((0, 0, 10, 4, 2)), rows.index((0, 2, 12, 4, 2))
    assert got[a, b] == 0
    # different buffers never overlap
    two = np.array([(0, 0, 8, 0, 0), (1, 0, 8, 0, 0)], np.uint64)
    out = np.zeros(4, np.uint8)
    probe().zs_overlap_matrix(two.ctypes.data, 2, out.ctypes.data)
    assert out.tolist() == [1, 0, 0, 1]


# ── 2. the declared footprints cover the real ones ────────────────────────────────────────────────────────────────────

def _run_oracle(oracle, ops, sizes, data, qweights=()):
    from zgml_amd import DeviceProgram, ProgramIO
    be = oracle.OracleBackend()
    prog = DeviceProgram(ops=list(ops), buffer_sizes=list(sizes), initial_uploads=[ProgramIO(i, d.copy()) for i, d in enumerate(data)],
                         qweights=list(qweights))
    h = be.compileProgram(prog)
    assert h, "oracle compile failed"
    try:
        be.executeProgram(h, [], [])
        return [be.buffer(h, i).copy() for i in range(len(sizes))]
    finally:
        be.freeProgram(h)


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_declared_footprints_cover_what_the_op_touches(oracle, kind):
    """One op on random buffers in the oracle: every element that changes lies in a declared write span, and changing every
    element outside the declared read and write spans leaves the op's results bit-identical."""
    size, n_bufs = 128, 4
    for seed in range(40):
        rng = np.random.default_rng(1000 * PC.KINDS.index(kind) + seed)
        op, bound = PC.random_op(rng, kind, n_bufs, size)
        qw = [PC.qmatmul_weight(rng)] if kind == "qmatmul" else []
        sizes = [size] * n_bufs
        _, spans, _ = schedule([op], sizes, seq_kv_bound=[bound] if bound else None)
        run_op = op
        if bound and kind.startswith("attention") and kind != "attention_kvq":
            run_op = op.with_(seq_kv=bound)  # the extents come from the bound, not from the op's current seq_kv
        data = [PC.random_values(rng, size) for _ in range(n_bufs)]
        after = _run_oracle(oracle, [run_op], sizes, data, qw)
        for b in range(n_bufs):
            changed = _bits(after[b]) != _bits(data[b])
            outside = changed & ~footprint(spans, 0, 1, b, size)
            assert not outside.any(), f"{kind} seed {seed}: {op} wrote buffer {b} at {np.flatnonzero(outside)[:8]} outside its spans"
        data2 = []
        for b in range(n_bufs):
            keep = footprint(spans, 0, None, b, size)
            d = PC.random_values(rng, size)
            d[keep] = data[b][keep]
            data2.append(d)
        after2 = _run_oracle(oracle, [run_op], sizes, data2, qw)
        for b in range(n_bufs):
            w = footprint(spans, 0, 1, b, size)
            bad = w & (_bits(after2[b]) != _bits(after[b]))
            assert not bad.any(), f"{kind} seed {seed}: {op} read outside its declared spans (buffer {b}, elements {np.flatnonzero(bad)[:8]})"


# ── 3. reordering by level changes nothing ─────────────────────────────────────────────────────────────────────────────

SEEDS = list(range(30))


@pytest.mark.parametrize("seed", SEEDS)
def test_level_order_equals_program_order(oracle, seed):
    ops, sizes, barriers, bounds = PC.random_program(seed)
    level, _, _ = schedule(ops, sizes, barriers, seq_kv_bound=bounds)
    for b in barriers:  # nothing crosses a barrier
        assert level[:b].max() < level[b:].min(), (b, level.tolist())
    rng = np.random.default_rng(seed + 7)
    data = [PC.random_values(rng, s) for s in sizes]
    want = _run_oracle(oracle, ops, sizes, data)
    for shuffle in range(4):
        order = []
        for lv in range(int(level.max()) + 1):
            idx = [i for i in range(len(ops)) if level[i] == lv]
            if shuffle == 0:
                idx.reverse()
            else:
                rng.shuffle(idx)
            order += idx
        got = _run_oracle(oracle, [ops[i] for i in order], sizes, data)
        for b in range(len(sizes)):
            assert np.array_equal(_bits(got[b]), _bits(want[b])), f"seed {seed} shuffle {shuffle}: buffer {b} differs (order {order})"


def test_random_programs_have_parallel_levels():
    """the generator makes programs the schedule can reorder at all (otherwise the test above proves nothing)"""
    widths = []
    for seed in SEEDS:
        ops, sizes, barriers, bounds = PC.random_program(seed)
        level, _, _ = schedule(ops, sizes, barriers, seq_kv_bound=bounds)
        widths.append(len(ops) / (int(level.max()) + 1))
    assert np.mean(widths) > 1.3, widths


# ── 4. dynamic_fields_in_bounds ────────────────────────────────────────────────────────────────────────────────────────

def in_bounds_per_op(ops, sizes, refreshed, seq_kv_bound=None):
    """dynamic_field_in_bounds for every op of `refreshed` against the schedule of `ops`"""
    arr, keep = ops_to_c(ops)
    ref, keep2 = ops_to_c(refreshed)
    sz = np.array(sizes, np.uint64)
    bound = np.array(seq_kv_bound, np.uint32) if seq_kv_bound is not None else None
    out = np.zeros(len(ops), np.uint8)
    probe().zs_dynamic_field_in_bounds(C.addressof(arr), len(ops), sz.ctypes.data, len(sizes), bound.ctypes.data if bound is not None else None,
                                       C.addressof(ref), out.ctypes.data)
    return [bool(v) for v in out]


def test_dynamic_fields_in_bounds_at_the_edges():
    from zgml_amd import DeviceOp
    dh, cols = 4, 8
    # two dynamic K stores into one cache buffer: slabs [0, 32) and [32, 64); the attention reads up to its compile-time seq_kv
    k0 = DeviceOp.slice_assign(0, 1, dh, 1, 0, 0, 1, dh, 0, 1, dh, dh)
    k1 = DeviceOp.slice_assign(0, 1, dh, 1, dh * cols, dh * cols, 1, dh, 0, 1, dh, dh)
    att = DeviceOp.attention(2, 1, 0, 0, 0, False, dh, 1, 3, 0.5, 0, 0, 0, 0, 0, 1, dh, 1, dh, 1, dh, 1, 1, 1, dh)
    ops, sizes = [k0, k1, att], [2 * dh * cols + 4, dh, dh]
    last = dh * cols - dh
    # (refreshed op list, the whole list is in bounds, the op that moved): one below, at and one past each edge
    for refreshed, want, moved in (([k0.with_(dst_offset=last - 1), k1, att], True, 0),
                                   ([k0.with_(dst_offset=last), k1, att], True, 0),                # the last column of slab 0
                                   ([k0.with_(dst_offset=last + 1), k1, att], False, 0),           # one element past it
                                   ([k0, k1.with_(dst_offset=dh * cols - 1), att], False, 1),      # one below slab 1's base
                                   ([k0, k1.with_(dst_offset=2 * dh * cols - 1), att], True, 1),
                                   ([k0, k1.with_(dst_offset=2 * dh * cols), att], True, 1),       # slab 1 runs to the buffer's end
                                   ([k0, k1.with_(dst_offset=2 * dh * cols + 1), att], False, 1),
                                   ([k0, k1, att.with_(seq_kv=2)], True, 2),
                                   ([k0, k1, att.with_(seq_kv=3)], True, 2),
                                   ([k0, k1, att.with_(seq_kv=4)], False, 2)):
        _, _, ok = schedule(ops, sizes, refreshed=refreshed)
        assert ok is want, refreshed
        per_op = in_bounds_per_op(ops, sizes, refreshed)  # the per-op function: only the op that moved can be out, and all() is the list's answer
        assert per_op == [want if i == moved else True for i in range(3)], (refreshed, per_op)
    # with a seq_kv bound above the op's value, the bound is the limit
    for kv, want in ((5, True), (6, True), (7, False)):
        refreshed = [k0, k1, att.with_(seq_kv=kv)]
        _, _, ok = schedule(ops, sizes, seq_kv_bound=[0, 0, 6], refreshed=refreshed)
        assert ok is want
        assert in_bounds_per_op(ops, sizes, refreshed, seq_kv_bound=[0, 0, 6]) == [True, True, want]


# ── 5. dyn_field: THE definition of an op's position-dependent word ────────────────────────────────────────────────────

def _dyn_field(op, poke=0xABCD1234):
    """(role, moves, base, stride, has_word, [at(0,1), at(0,4), at(5,1), at(5,4)], struct bytes before, after the poke, the C op)"""
    arr, keep = ops_to_c([op])
    before = bytes(arr[0])
    out = np.zeros(10, np.uint32)
    probe().zs_dyn_field(C.addressof(arr), poke, out.ctypes.data)
    assert out[9] == 1  # the const overload names the same word
    return int(out[0]), bool(out[1]), int(out[2]), int(out[3]), bool(out[4]), [int(v) for v in out[5:9]], before, bytes(arr[0]), arr[0]


@pytest.mark.parametrize("kind", PC.KINDS)
def test_dyn_field_of_every_kind(kind):
    """Every DeviceOp kind (the generator's sixteen variants cover the twelve reference kinds and the two quantised-KV extensions):
    only the two stores and the two attentions have a word; it aliases dst_offset / col / seq_kv; a store moves iff its
    patch_stride is not 0; at(pos, T) is base + pos * stride for a store and pos + T for an attention."""
    NONE, OFFSET, SEQ_KV = 0, 1, 2
    poke = 0xABCD1234
    op, _ = PC.random_op(np.random.default_rng(PC.KINDS.index(kind)), kind, 4, 128)
    variants = [op]
    if op.kind in ("slice_assign", "kvq_store"):  # stride 0 and stride non-zero, whatever the generator drew
        base = "dst_base_offset" if op.kind == "slice_assign" else "col_base"
        variants = [op.with_(patch_stride=0, **{base: 7}), op.with_(patch_stride=3, **{base: 7}), op.with_(patch_stride=16, **{base: 0})]
    for v in variants:
        role, moves, base, stride, has_word, at, before, after, c = _dyn_field(v, poke)
        if v.kind in ("slice_assign", "kvq_store"):
            b = v.dst_base_offset if v.kind == "slice_assign" else v.col_base
            assert (role, has_word, base, stride) == (OFFSET, True, b, v.patch_stride), v
            assert moves is (v.patch_stride != 0), v
            assert at == [b, b, b + 5 * v.patch_stride, b + 5 * v.patch_stride], v  # T plays no part
            field = c.u.slice_assign.dst_offset if v.kind == "slice_assign" else c.u.kvq_store.col
        elif v.kind in ("attention", "attention_kvq"):
            assert (role, has_word, base, stride, moves) == (SEQ_KV, True, 0, 0, True), v
            assert at == [1, 4, 6, 9], v
            field = c.u.attention.seq_kv if v.kind == "attention" else c.u.attention_kvq.seq_kv
        else:
            assert (role, has_word, base, stride, moves) == (NONE, False, 0, 0, False), v
            assert after == before, v  # nothing to write through
            continue
        assert field == poke, v  # written through the word, read from the field
        changed = [i for i in range(len(before)) if before[i] != after[i]]
        assert changed and max(changed) - min(changed) < 4, (v, changed)  # ... and from nothing else
