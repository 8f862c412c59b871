"""zgml_hip_kv_park / zgml_hip_kv_resume on the MI355X (zgml_amd/csrc/kv_park.hip): KV columns of every lane of a sequence into a
host blob and back. Bit contracts: a parked blob is the numpy model's blob (tests/kv_park_model.py, which tests/test_kv_park_host.py
holds to zgml_amd/csrc/kv_park.h) byte for byte; a resume puts exactly those bytes into the asked columns and leaves every other
byte of every KV buffer alone; an f32 run resumed into an int8 lane leaves what zgml_hip_kv_move leaves for f32 -> int8; every
refusal returns -1 with a prefixed text, before any launch, and changes nothing. End to end: a parked and resumed sequence decodes
the tokens of an uninterrupted one while its neighbour never notices, and a prompt parked once outlives its prefill plan and is
resumed into two slots of a new batched plan."""
import re
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from zgml_amd.program import ios_to_c
from tests import kv_park_model as M
from tests.kvq_cases import tiny64

pytestmark = pytest.mark.gpu
f32 = np.float32
PATTERN = 0xA5
ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"kKvmChunk = (\d+);", (ROOT / "zgml_amd" / "csrc" / "kv_copy.h").read_text()).group(1))  # values per workgroup


def cache_elems(n_cols, dh):
    return n_cols * dh // 4 + n_cols * (dh // 32)


def download(be, handle, buf, n_elems):
    out = np.zeros(n_elems, f32)
    capi.load_hip().zgml_hip_download_outputs(be.ctx, handle, ios_to_c([ProgramIO(buf, out)]), 1)
    assert not be.last_error(), be.last_error()
    return out


def upload(be, handle, buf, arr):
    arr = np.ascontiguousarray(arr, f32)
    capi.load_hip().zgml_hip_upload_inputs(be.ctx, handle, ios_to_c([ProgramIO(buf, arr)]), 1)
    assert not be.last_error(), be.last_error()


def holder(be, sizes, uploads=None):
    """a compiled program whose only purpose is to own buffers: one 1-element op per buffer keeps each of them live"""
    n = len(sizes)
    ops = [DeviceOp.elementwise("add", n, i, i, 1) for i in range(n)]
    prog = DeviceProgram(ops=ops, buffer_sizes=list(sizes) + [1], initial_uploads=[ProgramIO(i, a) for i, a in (uploads or {}).items()])
    h = be.compileProgram(prog)
    assert h, be.last_error()
    return h


def lanes_c(lanes):
    return (capi.KvLaneC * max(1, len(lanes)))(*[capi.KvLaneC(buf=b, d_head=dh, n_cols=nc, block_size=bs, offset=off) for b, off, dh, nc, bs in lanes])


def as_tuples(lanes):
    """KvLaneC array (Model.kv_lanes) -> [(buf, offset, d_head, n_cols, block_size)]"""
    return [(int(l.buf), int(l.offset), int(l.d_head), int(l.n_cols), int(l.block_size)) for l in lanes]


def park(be, h, lanes, col, n, flags=0, cap=None, blob=True, table=True):
    """-> (rc, blob): the blob has the size zgml_hip_kv_park_bytes says (at least a header's, so a refused call has room to miss)"""
    hip = capi.load_hip()
    arr = lanes_c(lanes)
    size = int(hip.zgml_hip_kv_park_bytes(arr, len(lanes), n, flags))
    out = np.full(max(size, M.HEADER), PATTERN, np.uint8)
    rc = hip.zgml_hip_kv_park(be.ctx, h, arr if table else None, len(lanes), col, n, flags, out.ctypes.data if blob else None, size if cap is None else cap)
    return rc, out[:size]


def resume(be, h, lanes, col, blob, nbytes=None, table=True):
    blob = np.ascontiguousarray(blob, np.uint8) if blob is not None else None
    return capi.load_hip().zgml_hip_kv_resume(be.ctx, h, lanes_c(lanes) if table else None, len(lanes), col, blob.ctypes.data if blob is not None else None,
                                              (blob.size if blob is not None else 0) if nbytes is None else nbytes)


def pattern(n_elems):
    return np.full(n_elems * 4, PATTERN, np.uint8).view(f32)


def random_bits(rng, n_elems):
    """arbitrary bit patterns (NaNs, infinities and denormals among them), with a negative zero, a denormal and an all-zero block"""
    img = rng.integers(0, 2 ** 32, n_elems, dtype=np.uint64).astype(np.uint32)
    img[0], img[1] = 0x80000000, 0x00000001
    if n_elems >= 96:
        img[32:64] = 0
    return img.view(f32)


def lane_columns(images, lane, col, n):
    """columns [col, col + n) of a lane out of the buffers' images: f32 [n, d_head], or (int8 [n, d_head], scales [n, d_head / 32])"""
    buf, off, dh, nc, bs = lane
    img = images[buf]
    if not bs:
        return img[off + col * dh:off + (col + n) * dh].reshape(n, dh)
    q = img.view(np.int8)[col * dh:(col + n) * dh].reshape(n, dh)
    sc0 = nc * dh // 4
    return q, img[sc0 + col * (dh // 32):sc0 + (col + n) * (dh // 32)].reshape(n, dh // 32)


def put_columns(images, lane, col, cols):
    buf, off, dh, nc, bs = lane
    img = images[buf]
    if not bs:
        n = cols.shape[0]
        img[off + col * dh:off + (col + n) * dh] = cols.ravel()
        return
    q, sc = cols
    n = q.shape[0]
    img.view(np.int8)[col * dh:(col + n) * dh] = q.ravel()
    sc0 = nc * dh // 4
    img[sc0 + col * (dh // 32):sc0 + (col + n) * (dh // 32)] = sc.ravel()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def round_trip(be, h, sizes, lanes, col, n, col2, rng, flags=0):
    """Fill every buffer with random bits, park [col, col + n) of `lanes` and hold the blob to the model; overwrite every buffer
    with the pattern, resume at col2 and hold every byte of every buffer to: the parked columns inside [col2, col2 + n) of the
    lanes, the pattern everywhere else. sizes: {buffer: f32 elements}."""
    images = {b: random_bits(rng, s) for b, s in sizes.items()}
    for b, img in images.items():
        upload(be, h, b, img)
    rc, blob = park(be, h, lanes, col, n, flags)
    assert rc == 0 and not be.last_error(), be.last_error()
    cols = [lane_columns(images, l, col, n) for l in lanes]
    want_blob = M.blob(lanes, cols, n, flags)
    assert blob.size == want_blob.size == M.layout(lanes, n, flags)[0]
    assert np.array_equal(blob, want_blob), (col, n, int(np.flatnonzero(blob != want_blob)[0]))
    for b, s in sizes.items():  # a park writes no lane
        assert same_bits(download(be, h, b, s), images[b]), b
    want = {b: pattern(s) for b, s in sizes.items()}
    for b, img in want.items():
        upload(be, h, b, img)
    assert resume(be, h, lanes, col2, blob) == 0 and not be.last_error(), be.last_error()
    blob[:] = 0  # (the blob has been consumed on return)
    for l, c in zip(lanes, cols):
        put_columns(want, l, col2, c)
    for b, s in sizes.items():
        got = download(be, h, b, s)
        assert same_bits(got, want[b]), (col, n, col2, b, int(np.flatnonzero(got.view(np.uint32) != want[b].view(np.uint32))[0]))


# ── round trips on model plans ─────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("plan", ["f32 single", "f32 batched", "int8 batched"])
def test_round_trip_to_the_bit_on_model_plans(hip_backend, plan):
    """tiny64 plans: the single-sequence f32 plan (all its lanes), and sequence 1 of three of a batched plan over f32 slabs / int8
    caches — whose neighbours' slots lie in the same buffers (f32) or in buffers of their own (int8) and keep their pattern, as
    does the stale tail behind the resumed columns."""
    be, rng, cfg = hip_backend, np.random.default_rng(11), tiny64()
    fns = llama.hip_backend_fns(be)
    if plan == "f32 single":
        m = llama.Model(cfg, llama.Q4_0)
        s = llama.Session(m, fns)
        lanes, every = as_tuples(m.kv_lanes()), as_tuples(m.kv_lanes())
    else:
        m = llama.BatchModel(cfg, 3, llama.Q4_0, kv_quant_block=32 if plan == "int8 batched" else 0)
        s = llama.BatchSession(m, fns, 3)
        lanes, every = as_tuples(m.kv_lanes(1)), as_tuples(m.kv_lanes())
    assert len(lanes) == 2 * cfg.n_layers * cfg.n_kv_heads
    sizes = {b: int(m.program.buffer_sizes[b]) for b in sorted({l[0] for l in every})}
    S = cfg.max_seq_len
    for col, n, col2 in [(0, S, 0), (5, 9, 5), (3, 1, 40), (7, 20, 0)]:
        round_trip(be, s.handle, sizes, lanes, col, n, col2, rng)
    # the wrappers are the same calls
    images = {b: random_bits(rng, sz) for b, sz in sizes.items()}
    for b, img in images.items():
        upload(be, s.handle, b, img)
    blob = s.park(6, col=2) if plan == "f32 single" else s.park(1, 6, col=2)
    assert isinstance(blob, np.ndarray) and blob.dtype == np.uint8
    assert np.array_equal(blob, M.blob(lanes, [lane_columns(images, l, 2, 6) for l in lanes], 6))
    s.resume(blob, col=9) if plan == "f32 single" else s.resume(1, blob.tobytes(), col=9)
    for l in lanes:
        put_columns(images, l, 9, lane_columns(images, l, 2, 6))
    for b, sz in sizes.items():
        assert same_bits(download(be, s.handle, b, sz), images[b]), b
    s.close(), m.close()


# ── column cuts on hand-sized lanes ────────────────────────────────────────────────────────────
def test_column_cuts(hip_backend):
    """Runs of exactly the kernel's chunk, one value (int8: one block) less and more, so the last workgroup of a lane has a full
    chunk, a chunk short of one value, and a single value; n = 1; odd columns; f32 lanes whose first moved byte is not 16-byte
    aligned — d_head 1 at an odd column, lanes at odd f32 offsets, which take the dword path, beside d_head 8 at an odd column —;
    lanes of one call that differ in d_head, form and n_cols; and a resume at another column than the park's."""
    be, rng = hip_backend, np.random.default_rng(12)
    # buffer 0: f32 lanes A (d_head 1, 16-byte aligned), A2 (d_head 1, odd offset), B (d_head 8, odd offset), E (d_head 8, aligned)
    nA, nA2, nB, nE = 2 * CHUNK + 40, 2 * CHUNK + 300, 1100, 150
    oA, oA2 = 4, 4 + nA + 5
    oA2 += 1 - oA2 % 2  # odd
    oB = oA2 + nA2 + 2
    oB += 1 - oB % 2
    oE = (oB + nB * 8 + 9) // 4 * 4
    size0 = oE + nE * 8 + 3
    A, A2, B, E = (0, oA, 1, nA, 0), (0, oA2, 1, nA2, 0), (0, oB, 8, nB, 0), (0, oE, 8, nE, 0)
    nC, nD = CHUNK // 32 + 44, CHUNK // 64 + 12
    Cq, Dq = (1, 0, 32, nC, 32), (2, 0, 64, nD, 32)
    sizes = {0: size0, 1: cache_elems(nC, 32) + 3, 2: cache_elems(nD, 64) + 3}
    assert oA % 4 == 0 and oE % 4 == 0 and oA2 % 2 == 1 and oB % 2 == 1
    h = holder(be, [sizes[b] for b in range(3)])
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):  # d_head 1: values = columns
        round_trip(be, h, sizes, [A, A2], 3, n, 4, rng)
    round_trip(be, h, sizes, [A, A2], 0, 2 * CHUNK + 7, 32, rng)  # more than two chunks per lane
    for n in (CHUNK // 32 - 1, CHUNK // 32, CHUNK // 32 + 1):  # int8, d_head 32: one block less, the chunk, one block more
        round_trip(be, h, sizes, [Cq], 1, n, 43, rng)
    mixed = [B, Cq, Dq, E, A]
    for col, n, col2 in [(1, 1, 2), (3, 7, 3), (5, CHUNK // 64 - 1, 0), (1, CHUNK // 64, 11), (0, CHUNK // 64 + 1, 3), (7, 128, 8)]:
        assert col + n <= nD and col2 + n <= nD
        round_trip(be, h, sizes, mixed, col, n, col2, rng)
    be.freeProgram(h)


# ── f32 -> int8 ────────────────────────────────────────────────────────────────────────────────
def finite_cols(rng, n_cols, dh):
    c = ((rng.random((n_cols, dh)) - 0.5) * 2).astype(f32) * (10.0 ** rng.integers(-3, 3, (n_cols, 1))).astype(f32)
    c[1 % n_cols, :32] = 0.0                 # an all-zero block
    c[2 % n_cols, 3], c[2 % n_cols, 40 % dh] = -0.0, 1e-41  # a negative zero and a denormal
    return c


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_f32_runs_into_int8_lanes_equal_kv_move(hip_backend, dh):
    """An f32 source (two lanes: 16-byte aligned, and at an odd f32 offset) goes into three slots of int8 caches: by
    zgml_hip_kv_move; parked plain and resumed (quantised by the resume); parked with ZGML_KV_PARK_INT8 (quantised by the park) and
    resumed. All three slots hold the same bytes and scales, and everything else of their buffers keeps its pattern. The
    quantised blob is the model's blob byte for byte, its size the model's: 0.28 of the plain one at d_head 128."""
    be, rng = hip_backend, np.random.default_rng(300 + dh)
    n_src, n_dst = 40, 48
    src_off = [0, n_src * dh + 1]
    cols = [finite_cols(rng, n_src, dh) for _ in src_off]
    src_img = np.zeros(src_off[1] + n_src * dh, f32)
    for o, c in zip(src_off, cols):
        src_img[o:o + n_src * dh] = c.ravel()
    hs = holder(be, [src_img.size], {0: src_img})
    src = [(0, o, dh, n_src, 0) for o in src_off]
    ce = cache_elems(n_dst, dh) + 3
    for src_col, dst_col, n in [(3, 5, 1), (3, 5, 7), (1, 0, 33), (0, 0, n_src)]:
        hd = holder(be, [ce] * 6, {b: pattern(ce) for b in range(6)})
        slot = [[(2 * k + i, 0, dh, n_dst, 32) for i in (0, 1)] for k in range(3)]
        assert capi.load_hip().zgml_hip_kv_move(be.ctx, hd, lanes_c(slot[0]), hs, lanes_c(src), 2, src_col, dst_col, n) == 0
        rc, plain = park(be, hs, src, src_col, n)
        assert rc == 0 and resume(be, hd, slot[1], dst_col, plain) == 0, be.last_error()
        rc, small = park(be, hs, src, src_col, n, M.INT8)
        assert rc == 0 and resume(be, hd, slot[2], dst_col, small) == 0, be.last_error()
        assert not be.last_error(), be.last_error()
        moved = [c[src_col:src_col + n] for c in cols]
        assert np.array_equal(plain, M.blob(src, moved, n))
        want_small = M.blob(src, moved, n, M.INT8)
        assert small.size == want_small.size == M.layout(src, n, M.INT8)[0]
        assert np.array_equal(small, want_small)
        if dh == 128 and n == n_src:
            assert abs(small.size / plain.size - 0.28125) < 0.01
        got = [download(be, hd, b, ce) for b in range(6)]
        untouched = pattern(ce)
        for i in (0, 1):
            assert not same_bits(got[i], untouched)  # (the move wrote something)
            assert same_bits(got[i], got[2 + i]) and same_bits(got[i], got[4 + i]), (src_col, dst_col, n, i)
            q, sc = M.quantise(moved[i])  # and, since these values are finite, the model's columns
            want = {0: untouched.copy()}
            put_columns(want, (0, 0, dh, n_dst, 32), dst_col, (q, sc))
            assert same_bits(got[i], want[0])
        be.freeProgram(hd)
    be.freeProgram(hs)


# ── end to end ─────────────────────────────────────────────────────────────────────────────────
def prompt(seed, T, vocab):
    return [(49 * seed + 5 * j + 1) % vocab for j in range(T)]


@pytest.mark.parametrize("kvq", [0, 32])
def test_a_parked_sequence_continues_as_if_never_interrupted(hip_backend, kvq):
    """Two sequences in the greedy batched resident loop. Both decode 8 tokens; sequence 0 is parked; another prompt is prefilled,
    admitted into slot 0 and decoded 4 steps (it overwrites slot 0's columns 0..7) while sequence 1 goes on; the blob comes back
    into slot 0 and both decode 8 more. Sequence 0's 16 tokens are those of an uninterrupted run, and sequence 1's 20 tokens those
    of a run in which slot 0 was never touched."""
    be, B, cfg = hip_backend, 2, tiny64()
    fns = llama.hip_backend_fns(be)
    base = llama.Model(cfg, llama.Q4_0)
    bm = llama.BatchModel(cfg, B, like=base, kv_quant_block=kvq)
    first = [5, 90]
    ref_s = llama.BatchSession(bm, fns, B)
    ref_s.resident_setup(be)
    ref = ref_s.resident_decode_batch(first, [0, 0], [16, 20])
    ref_s.close()
    s = llama.BatchSession(bm, fns, B)
    s.resident_setup(be)
    a = s.resident_decode_batch(first, [0, 0], 8)
    blob = s.park(0, 8)
    T = 4
    mp = llama.Model(cfg, llama.Q4_0, token_len=T)
    ph = llama.Session(mp, fns)
    t_other, _ = ph.prefill(prompt(3, T, cfg.vocab_size), 0)
    s.admit(0, ph, T)
    b = s.resident_decode_batch([t_other, int(a[1, 7])], [T, 8], 4)
    assert b[0].tolist() != ref[0, 8:12].tolist()  # (slot 0 really ran something else)
    s.resume(0, blob)
    c = s.resident_decode_batch([int(a[0, 7]), int(b[1, 3])], [8, 12], 8)
    assert not be.last_error(), be.last_error()
    assert a[0].tolist() + c[0].tolist() == ref[0, :16].tolist()
    assert a[1].tolist() + b[1].tolist() + c[1].tolist() == ref[1, :20].tolist()
    ph.close(), mp.close(), s.close(), bm.close(), base.close()


@pytest.mark.parametrize("kvq", [0, 32])
def test_a_parked_prompt_outlives_its_prefill_plan(hip_backend, kvq):
    """Prompt cache: a 6-token prompt is prefilled on an f32 T-token plan and parked; a batched session admits it directly into
    slot 1 and decodes 6 tokens (the reference); prefill plan and that session are freed; a NEW batched session resumes the blob
    into slots 0 and 2 (quantised on the way when its caches are int8) and both decode the reference's tokens."""
    be, B, cfg, T, n = hip_backend, 3, tiny64(), 6, 6
    fns = llama.hip_backend_fns(be)
    base = llama.Model(cfg, llama.Q4_0)
    mp = llama.Model(cfg, llama.Q4_0, token_len=T)
    ph = llama.Session(mp, fns)
    t0, _ = ph.prefill(prompt(2, T, cfg.vocab_size), 0)
    blob = ph.park(T)
    bm = llama.BatchModel(cfg, B, like=base, kv_quant_block=kvq)
    s1 = llama.BatchSession(bm, fns, B)
    s1.resident_setup(be)
    s1.admit(1, ph, T)
    want = s1.resident_decode_batch([t0] * B, [T] * B, n)[1]
    be.synchronize()
    s1.close(), ph.close(), mp.close()
    kept = blob.tobytes()  # (what an application would have written to a file)
    del blob
    s2 = llama.BatchSession(bm, fns, B)
    s2.resident_setup(be)
    s2.resume(0, kept)
    s2.resume(2, kept)
    got = s2.resident_decode_batch([t0] * B, [T] * B, n)
    assert not be.last_error(), be.last_error()
    assert got[0].tolist() == want.tolist() and got[2].tolist() == want.tolist()
    s2.close(), bm.close(), base.close()


# ── refusals and the empty blob ────────────────────────────────────────────────────────────────
def test_refusals_return_before_any_launch_and_change_nothing(hip_backend):
    be, hip = hip_backend, capi.load_hip()
    dh, nc = 64, 16
    ce = cache_elems(nc, dh)
    # buffers: 0 an f32 slab (two lanes' worth), 1 / 2 int8 caches, 3 an f32 slab of d_head 80, 4 dead (no op references it)
    sizes = [2 * nc * dh, ce, ce, nc * 80]
    n = len(sizes)
    rng = np.random.default_rng(5)
    images = {b: random_bits(rng, s) for b, s in enumerate(sizes)}
    prog = DeviceProgram(ops=[DeviceOp.elementwise("add", n + 1, i, i, 1) for i in range(n)], buffer_sizes=sizes + [nc * dh, 1],
                         initial_uploads=[ProgramIO(b, img) for b, img in images.items()])
    h = be.compileProgram(prog)
    F, F2, Q, Q2, W = (0, 0, dh, nc, 0), (0, nc * dh, dh, nc, 0), (1, 0, dh, nc, 32), (2, 0, dh, nc, 32), (3, 0, 80, nc, 0)

    def refused(rc, prefix, word):
        err = be.last_error()
        assert rc == -1 and err.startswith(prefix) and word in err, (word, rc, err)
        hip.zgml_hip_clear_error(be.ctx)

    park_bad = [  # (word, lanes, col, n, flags, keywords of park())
        ("dead", [(4, 0, dh, nc, 0)], 0, 4, 0, {}),
        ("no such", [(9, 0, dh, nc, 0)], 0, 4, 0, {}),
        ("block_size", [(1, 0, dh, nc, 16)], 0, 4, 0, {}),
        ("must not be 0", [(0, 0, 0, nc, 0)], 0, 4, 0, {}),
        ("must not be 0", [(0, 0, dh, 0, 0)], 0, 4, 0, {}),
        ("n_cols", [F, Q], 13, 4, 0, {}),                        # columns beyond n_cols
        ("n_cols", [F], 0xFFFFFFFF, 2, 0, {}),                   # (col + n wraps in 32 bits)
        ("n_cols", [F], 0, nc + 1, 0, {}),
        ("extent", [(3, 1, 80, nc, 0)], 0, 4, 0, {}),            # an f32 lane that ends past its buffer
        ("extent", [(1, 0, dh, nc + 1, 32)], 0, 4, 0, {}),       # an int8 lane larger than its buffer
        ("d_head % 32", [(1, 0, 48, nc, 32)], 0, 4, 0, {}),
        ("offset", [(1, 4, dh, nc - 1, 32)], 0, 4, 0, {}),       # an int8 lane with an offset
        ("KV_PARK_INT8", [F, W], 0, 4, M.INT8, {}),         # the flag on an f32 lane of d_head 80
        ("flags", [F], 0, 4, 2, {}),
        ("cap below", [F, Q], 0, 4, 0, {"cap": M.layout([F, Q], 4)[0] - 1}),
        ("cap below", [F], 0, 0, 0, {"cap": M.HEADER - 1}),      # (an empty blob needs its header's room)
        ("no blob", [F], 0, 4, 0, {"blob": False}),
        ("lane records", [F], 0, 4, 0, {"table": False}),
    ]
    for word, lanes, col, cnt, flags, kw in park_bad:
        if not kw.get("table", True):  # (the size of a NULL table is 0: hand the call room of its own)
            kw = dict(kw, cap=1 << 20)
        rc, blob = park(be, h, lanes, col, cnt, flags, **kw)
        refused(rc, "kv_park:", word)
        assert np.all(blob == PATTERN)  # (nothing was written into the blob either)
    rc, good = park(be, h, [F, Q], 2, 4)
    assert rc == 0 and not be.last_error(), be.last_error()
    rc, good_q = park(be, h, [F], 2, 4, M.INT8)
    assert rc == 0

    def patched(blob, dt, field, value, base=0):
        out = blob.copy()
        out[base:base + dt.itemsize].view(dt)[field] = value
        return out

    resume_bad = [  # (word, lanes, col, blob, keywords of resume())
        ("dead", [(4, 0, dh, nc, 0), Q], 0, good, {}),
        ("n_cols", [F, Q], 13, good, {}),
        ("n_cols", [F, Q], 0xFFFFFFFE, good, {}),
        ("extent", [(0, nc * dh + 1, dh, nc, 0), Q], 0, good, {}),
        ("magic", [F, Q], 0, patched(good, M.HEADER_DT, "magic", 0), {}),
        ("version", [F, Q], 0, patched(good, M.HEADER_DT, "version", 7), {}),
        ("differ from the header's total", [F, Q], 0, good, {"nbytes": good.size - 16}),
        ("differ from the header's total", [F, Q], 0, np.concatenate([good, good[:16]]), {}),
        ("below a header", [F, Q], 0, good, {"nbytes": 8}),
        ("not the layout's", [F, Q], 0, patched(good, M.RECORD_DT, "offset", 1 << 40, M.HEADER + M.RECORD), {}),  # a directory that points far away
        ("not the layout's", [F, Q], 0, patched(good, M.HEADER_DT, "n", 5), {}),
        ("n_lanes differs", [F], 0, good, {}),
        ("n_lanes differs", [F, Q, Q2], 0, good, {}),
        ("d_head differs", [(3, 0, 80, nc, 0), Q], 0, good, {}),
        ("int8 -> f32", [F, F2], 0, park(be, h, [Q, F], 2, 4)[1], {}),                                   # the blob's lane 0 is an int8 run
        ("int8 -> f32", [F], 0, good_q, {}),
        ("overlapping", [F, F], 0, park(be, h, [F, F2], 0, 4)[1], {}),                                   # a lane listed twice
        ("overlapping", [F, (0, 2 * dh, dh, nc - 2, 0)], 0, park(be, h, [F, F2], 0, 4)[1], {}),          # columns [0, 4) meet [2, 6)
        ("overlapping", [Q, Q], 3, park(be, h, [Q, Q2], 0, 4)[1], {}),
        ("no blob", [F, Q], 0, None, {}),
        ("lane records", [F, Q], 0, good, {"table": False}),
    ]
    assert not be.last_error(), be.last_error()
    for word, lanes, col, blob, kw in resume_bad:
        refused(resume(be, h, lanes, col, blob, **kw), "kv_resume:", word)
    # no call above has changed a KV byte
    for b, img in images.items():
        assert same_bits(download(be, h, b, sizes[b]), img), b
    # a valid call still works: columns [2, 6) of F and Q into columns [7, 11) of F2 and Q2
    assert resume(be, h, [F2, Q2], 7, good) == 0
    be.synchronize()
    assert not be.last_error(), be.last_error()
    for src, dst in ((F, F2), (Q, Q2)):
        put_columns(images, dst, 7, lane_columns({b: i.copy() for b, i in images.items()}, src, 2, 4))
    for b, img in images.items():
        assert same_bits(download(be, h, b, sizes[b]), img), b
    be.freeProgram(h)


def test_empty_blob(hip_backend):
    """n == 0 or n_lanes == 0: 0, no error, whatever the lanes say; the park writes the bare header, which a resume accepts and
    ignores."""
    be = hip_backend
    img = random_bits(np.random.default_rng(6), 64 * 8)
    h = holder(be, [img.size], {0: img})
    F, junk = (0, 0, 64, 8, 0), (9, 3, 0, 0, 7)
    for lanes, n in [([F], 0), ([junk], 0), ([], 5)]:
        rc, blob = park(be, h, lanes, 3, n)
        assert rc == 0 and not be.last_error(), be.last_error()
        assert np.array_equal(blob, M.head([], 0)) and blob.size == M.HEADER
        assert resume(be, h, [F], 2, blob) == 0 and resume(be, h, [junk], 0, blob) == 0 and resume(be, h, [], 0, blob) == 0
    assert not be.last_error(), be.last_error()
    assert same_bits(download(be, h, 0, img.size), img)
    be.freeProgram(h)
