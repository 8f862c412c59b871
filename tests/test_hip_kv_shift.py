"""zgml_hip_kv_shift on the MI355X (zgml_amd/csrc/kv_shift.hip): the context shift of KV lanes in place, in one launch. Bit
contracts against the numpy model of tests/kv_shift_model.py (which tests/test_kv_shift_host.py holds to zgml_amd/csrc/kv_shift.h):
moved K columns are the model's rotated (int8: requantised) columns, moved V columns are copies, and every other byte of every
touched buffer keeps its pattern; two calls are the model applied twice; every refusal returns -1 with a text and leaves nothing
sticky; and end to end against the oracle — a sequence decoded past max_seq_len, one sequence of a batch shifted alone, and the
resident loop against vtable stepping from the shifted state."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from zgml_amd.program import ios_to_c
from tests import kv_shift_model as M
from tests.kvq_cases import KVQ_TOL, decisive, tiny64

pytestmark = pytest.mark.gpu
f32 = np.float32
PATTERN = 0xA5
F32_TOL = 2e-4  # of the row's largest magnitude: the f32 plans' bound (tests/test_hip_llama.py)


def cache_elems(n_cols, dh):
    return n_cols * dh // 4 + n_cols * (dh // 32)


def download(be, handle, buf, n_elems):
    out = np.zeros(n_elems, f32)
    capi.load_hip().zgml_hip_download_outputs(be.ctx, handle, ios_to_c([ProgramIO(buf, out)]), 1)
    assert not be.last_error(), be.last_error()
    return out


def holder(be, sizes, uploads):
    """a compiled program whose only purpose is to own buffers: one 1-element op per buffer keeps each of them live"""
    n = len(sizes)
    ops = [DeviceOp.elementwise("add", n, i, i, 1) for i in range(n)]
    prog = DeviceProgram(ops=ops, buffer_sizes=list(sizes) + [1], initial_uploads=[ProgramIO(i, a) for i, a in uploads.items()])
    h = be.compileProgram(prog)
    assert h, be.last_error()
    return h


def lanes_c(lanes):
    return (capi.KvLaneC * max(1, len(lanes)))(*[capi.KvLaneC(buf=b, d_head=dh, n_cols=nc, block_size=bs, offset=off) for b, off, dh, nc, bs in lanes])


def kv_shift(be, h, lanes, rotate, keep, discard, n_filled, c, s, n_lanes=None):
    f32p = C.POINTER(C.c_float)
    rot = (C.c_uint8 * max(1, len(rotate)))(*rotate) if rotate is not None else None
    return capi.load_hip().zgml_hip_kv_shift(be.ctx, h, lanes_c(lanes) if lanes is not None else None, rot, len(lanes) if n_lanes is None else n_lanes, keep,
                                             discard, n_filled, c.ctypes.data_as(f32p) if c is not None else None,
                                             s.ctypes.data_as(f32p) if s is not None else None)


def pattern(n_elems):
    return np.full(n_elems * 4, PATTERN, np.uint8).view(f32)


def rounds():
    rv, cb = C.c_uint32(0), C.c_uint32(0)
    capi.load_hip().zgml_hip_kv_shift_rounds(C.byref(rv), C.byref(cb))
    return int(rv.value), int(cb.value)


def rows(oracle, dh, discard, max_seq):
    cos, sin = oracle.rope_tables(dh, max(max_seq, discard + 1))
    return M.shift_rows(cos, sin, discard)


def rand_cols(rng, n, dh):
    c = ((rng.random((n, dh)) - 0.5) * 2).astype(f32) * (10.0 ** rng.integers(-2, 3, (n, 1))).astype(f32)
    if n > 2:
        c[n - 1, :32] = 0.0             # an all-zero block
        c[n - 2, dh // 2 + 1] = 4096.0  # the column's maximum in the `hi` half
    return c


CASES = [(0, 1, 2), (4, 8, 48), (3, 5, 41), (0, 47, 48), (4, 44, 48)]  # (keep, discard, n_filled) at n_cols 48; the last moves nothing


def long_case(dh, int8):
    """(n_cols, keep, discard, n_filled): at least three rounds of the kernel's loop on every path, the last one partial (5 columns
    more than whole rounds of either size), heavily overlapping (discard 7)"""
    rot_vals, copy_bytes = rounds()
    vals = max(rot_vals, copy_bytes if int8 else copy_bytes // 4)
    n_move = 3 * (-(-vals // dh)) + 5
    return 3 + 7 + n_move + 2, 3, 7, 3 + 7 + n_move


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_f32_lanes_equal_the_model_and_nothing_else_changes(hip_backend, oracle, dh):
    """One slab, four lanes per call (K V K V): the first pair 16-byte aligned, the second at an odd f32 offset (the dword paths);
    pattern floats between, before and behind the lanes and in every lane's stale tail."""
    be, rng = hip_backend, np.random.default_rng(dh)
    for n_cols, keep, discard, n_filled in [(48,) + c for c in CASES] + [long_case(dh, False)]:
        lane = n_cols * dh
        offs = [8, 8 + lane + 4, 8 + 2 * lane + 4 + 5, 8 + 3 * lane + 4 + 5 + 2]  # f32 offsets: 8, 12 mod 4 = 0; then odd, odd
        assert offs[0] % 4 == 0 and offs[1] % 4 == 0 and offs[2] % 2 == 1 and offs[3] % 2 == 1
        total = offs[3] + lane + 7
        img = pattern(total)
        for o in offs:
            img[o:o + n_filled * dh] = rand_cols(rng, n_filled, dh).ravel()
        c, s = rows(oracle, dh, discard, 64)
        h = holder(be, [total], {0: img})
        rc = kv_shift(be, h, [(0, o, dh, n_cols, 0) for o in offs], [1, 0, 1, 0], keep, discard, n_filled, c, s)
        assert rc == 0 and not be.last_error(), be.last_error()
        got = download(be, h, 0, total)
        want = img.copy()
        for i, o in enumerate(offs):
            want[o:o + lane] = M.shift_f32(img[o:o + lane].reshape(n_cols, dh), keep, discard, n_filled, i % 2 == 0, c, s).ravel()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n_cols, keep, discard, n_filled)
        if n_filled - keep - discard > 0:
            assert not np.array_equal(want, img)
        be.freeProgram(h)


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_int8_lanes_equal_the_model_and_nothing_else_changes(hip_backend, oracle, dh):
    """Four caches per call (K V K V), each three floats longer than its cache; bytes and scales of the columns in use are
    arbitrary (the K caches of the second pair are quantised columns with a zero block and a maximum in the `hi` half), the stale
    tail's bytes and scales are pattern."""
    be, rng = hip_backend, np.random.default_rng(100 + dh)
    bpc = dh // 32
    for n_cols, keep, discard, n_filled in [(48,) + c for c in CASES] + [long_case(dh, True)]:
        ce = cache_elems(n_cols, dh) + 3
        imgs = []
        for b in range(4):
            img = pattern(ce)
            q, sc = M.split_cache(img, n_cols, dh)
            if b < 2:
                q[:n_filled] = rng.integers(-128, 128, (n_filled, dh), dtype=np.int64).astype(np.int8)
                sc[:n_filled] = rng.random((n_filled, bpc)).astype(f32) + f32(0.01)
            else:
                q[:n_filled], sc[:n_filled] = M.quantise(rand_cols(rng, n_filled, dh))
            imgs.append(img)
        c, s = rows(oracle, dh, discard, 64)
        h = holder(be, [ce] * 4, dict(enumerate(imgs)))
        rc = kv_shift(be, h, [(b, 0, dh, n_cols, 32) for b in range(4)], [1, 0, 1, 0], keep, discard, n_filled, c, s)
        assert rc == 0 and not be.last_error(), be.last_error()
        for b in range(4):
            got = download(be, h, b, ce)
            want = M.shift_cache_image(imgs[b].copy(), n_cols, dh, keep, discard, n_filled, b % 2 == 0, c, s)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n_cols, keep, discard, n_filled, b)
        be.freeProgram(h)


@pytest.mark.parametrize("kvq", [0, 32])
def test_two_calls_are_the_model_applied_twice(hip_backend, oracle, kvq):
    be, rng, dh, n_cols = hip_backend, np.random.default_rng(5 + kvq), 64, 48
    c, s = rows(oracle, dh, 8, 64)
    if kvq:
        ce = cache_elems(n_cols, dh)
        imgs = []
        for _ in range(2):
            img = np.zeros(ce, f32)
            q, sc = M.split_cache(img, n_cols, dh)
            q[:], sc[:] = M.quantise(rand_cols(rng, n_cols, dh))
            imgs.append(img)
        h = holder(be, [ce, ce], dict(enumerate(imgs)))
        lanes = [(b, 0, dh, n_cols, 32) for b in range(2)]
        want = [M.shift_cache_image(M.shift_cache_image(imgs[b].copy(), n_cols, dh, 4, 8, 48, b == 0, c, s), n_cols, dh, 4, 8, 40, b == 0, c, s) for b in range(2)]
    else:
        imgs = [rand_cols(rng, n_cols, dh).ravel() for _ in range(2)]
        h = holder(be, [n_cols * dh] * 2, dict(enumerate(imgs)))
        lanes = [(b, 0, dh, n_cols, 0) for b in range(2)]
        want = [M.shift_f32(M.shift_f32(imgs[b].reshape(n_cols, dh), 4, 8, 48, b == 0, c, s), 4, 8, 40, b == 0, c, s).ravel() for b in range(2)]
    assert kv_shift(be, h, lanes, [1, 0], 4, 8, 48, c, s) == 0 and kv_shift(be, h, lanes, [1, 0], 4, 8, 40, c, s) == 0
    for b in range(2):
        got = download(be, h, b, want[b].size)
        assert np.array_equal(got.view(np.uint32), want[b].view(np.uint32)), b
    assert not be.last_error(), be.last_error()
    be.freeProgram(h)


def test_refusals_leave_nothing_sticky(hip_backend, oracle):
    be, hip = hip_backend, capi.load_hip()
    dh, nc = 64, 16
    ce = cache_elems(nc, dh)
    # buffers: 0 an f32 slab (two lanes' worth), 1 / 2 int8 caches, 3 an f32 slab, 4 an int8 cache of d_head 96, 5 dead (no op references it)
    sizes = [2 * nc * dh, ce, ce, nc * dh, cache_elems(nc, 96)]
    n = len(sizes)
    img = ((np.random.default_rng(1).random(2 * nc * dh) - 0.5) * 2).astype(f32)
    prog = DeviceProgram(ops=[DeviceOp.elementwise("add", n + 1, i, i, 1) for i in range(n)], buffer_sizes=sizes + [nc * dh, 1],
                         initial_uploads=[ProgramIO(0, img)])
    h = be.compileProgram(prog)
    c, s = rows(oracle, dh, 4, 64)
    F, F2, Q = (0, 0, dh, nc, 0), (0, nc * dh, dh, nc, 0), (1, 0, dh, nc, 32)
    bad = [  # (word, lanes, rotate, keep, discard, n_filled, c, s)
        ("dead", [(5, 0, dh, nc, 0)], [1], 2, 4, nc, c, s),             # a dead (elided) buffer
        ("no such", [(9, 0, dh, nc, 0)], [1], 2, 4, nc, c, s),          # a buffer id outside the program
        ("block_size", [(1, 0, dh, nc, 16)], [1], 2, 4, nc, c, s),      # block size other than 0 / 32
        ("must not be 0", [(0, 0, 0, nc, 0)], [1], 2, 4, nc, c, s),     # d_head 0
        ("must not be 0", [(0, 0, dh, 0, 0)], [1], 2, 4, 7, c, s),      # n_cols 0
        ("extent", [(3, 1, dh, nc, 0)], [1], 2, 4, nc, c, s),           # an f32 lane that ends past its buffer
        ("extent", [(1, 0, dh, nc + 1, 32)], [1], 2, 4, nc, c, s),      # an int8 lane larger than its buffer
        ("d_head % 32", [(1, 0, 48, nc, 32)], [1], 2, 4, nc, c, s),
        ("offset", [(1, 4, dh, nc - 1, 32)], [1], 2, 4, nc - 1, c, s),  # an int8 lane with an offset
        ("odd", [(0, 0, 63, nc, 0)], [1], 2, 4, nc, c, s),              # d_head odd
        ("differs", [F, (3, 0, 32, nc, 0)], [1, 0], 2, 4, nc, c, s),    # differing d_head across lanes
        ("d_head % 64", [(4, 0, 96, nc, 32)], [1], 2, 4, nc, c, s),     # an int8 K lane whose pairs straddle blocks
        ("exceeds n_filled", [F], [1], 9, 4, 12, c, s),                 # keep + discard > n_filled
        ("exceeds n_filled", [F], [1], 0xFFFFFFFF, 2, 12, c, s),        # (keep + discard wraps in 32 bits)
        ("n_cols", [F], [1], 2, 4, nc + 1, c, s),                       # n_filled > n_cols
        ("n_cols", [F, Q], [1, 1], 2, 4, 0xFFFFFFFF, c, s),
        ("row", [F], [1], 2, 4, nc, None, s),                           # null rows
        ("row", [F], [1], 2, 4, nc, c, None),
        ("meet", [F, F], [1, 0], 2, 4, nc, c, s),                       # a lane listed twice
        ("meet", [F, (0, nc * dh - dh, dh, nc, 0)], [1, 0], 2, 4, nc, c, s),  # two lanes that overlap by one column
        ("meet", [Q, F, Q], [1, 1, 0], 2, 4, nc, c, s),
    ]
    for word, lanes, rot, keep, discard, n_filled, cc, ss in bad:
        assert kv_shift(be, h, lanes, rot, keep, discard, n_filled, cc, ss) == -1, word
        err = be.last_error()
        assert err.startswith("kv_shift:") and word in err, (word, err)
        hip.zgml_hip_clear_error(be.ctx)
    assert kv_shift(be, h, None, None, 2, 4, nc, c, s, n_lanes=1) == -1 and "lane" in be.last_error()  # no lane table
    hip.zgml_hip_clear_error(be.ctx)
    # nothing to do: 0 and no error, whatever the lanes say
    junk = [(9, 0, dh, nc, 7)]
    assert kv_shift(be, h, junk, [1], 2, 0, nc, c, s) == 0 and kv_shift(be, h, [], [], 2, 4, nc, c, s) == 0 and kv_shift(be, h, junk, [1], 2, 4, 6, c, s) == 0
    assert not be.last_error()
    # a valid call still works, and does what the model says
    before = download(be, h, 0, 2 * nc * dh)
    assert np.abs(before).max() > 0.5
    assert kv_shift(be, h, [F, F2], [1, 0], 2, 4, nc, c, s) == 0
    be.synchronize()
    assert not be.last_error(), be.last_error()
    got = download(be, h, 0, 2 * nc * dh)
    want = np.concatenate([M.shift_f32(before[:nc * dh].reshape(nc, dh), 2, 4, nc, True, c, s).ravel(),
                           M.shift_f32(before[nc * dh:].reshape(nc, dh), 2, 4, nc, False, c, s).ravel()])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    be.freeProgram(h)


# ── end to end ───────────────────────────────────────────────────────────────────────────────
def forced(seed, j, vocab):
    return (49 * seed + 5 * j + 1) % vocab


def oracle_shift(ob, handle, lanes, keep, discard, n_filled, c, s, rotate=True):
    """the numpy model on the oracle's own buffers (K | V innermost: every even lane is a K lane)"""
    for i, l in enumerate(lanes):
        buf = ob.buffer(handle, l.buf)
        is_k = i % 2 == 0
        if l.block_size:
            M.shift_cache_image(buf, l.n_cols, l.d_head, keep, discard, n_filled, is_k and rotate, c, s)
        else:
            view = buf[l.offset:l.offset + l.n_cols * l.d_head].reshape(l.n_cols, l.d_head)
            view[:] = M.shift_f32(view, keep, discard, n_filled, is_k and rotate, c, s)


def check_row(tag, l_hip, l_ref, t_hip, t_ref, tol, bad):
    rel = float(np.abs(l_hip - l_ref).max() / np.abs(l_ref).max())
    dec = decisive(l_ref)
    print(f"{tag}: rel {rel:.3g} decisive {dec} tokens {int(t_hip)} {int(t_ref)}")
    if not np.isfinite(l_hip).all() or rel > tol or (dec and int(t_hip) != int(t_ref)):
        bad.append((tag, rel, int(t_hip), int(t_ref)))
    return rel


@pytest.mark.parametrize("kvq", [0, 32])
def test_generation_past_max_seq_matches_the_oracle(hip_backend, oracle, kvq):
    """tiny64 (max_seq 64): both sides step teacher-forced varied tokens through positions 0..63 until the cache is full, shift
    (keep 4, discard 28) — the device through Session.shift, the oracle through the numpy model on its own buffers — and step 28
    more forced tokens from position 36: generation past max_seq_len. Every row's logits within the project's bar (f32: 2e-4 of
    the row's largest magnitude; int8: KVQ_TOL), equal greedy tokens on the decisive rows. f32 only, a CPU-side control: the
    oracle with an UNROTATED move differs from the rotated oracle by more than twice the bar on at least one row, so these logits
    can witness a missing rotation (at the int8 bar they cannot: the bit-level cache tests above are the witnesses there)."""
    be, seed = hip_backend, 1
    cfg = tiny64()
    cfg.kv_quant_block = kvq
    tol = KVQ_TOL if kvq else F32_TOL
    S, V, keep, discard = cfg.max_seq_len, cfg.vocab_size, 4, 28
    assert S == 64
    m = llama.Model(cfg, llama.Q4_0)
    ob = oracle.OracleBackend()
    s_hip, s_ref = llama.Session(m, llama.hip_backend_fns(be)), llama.Session(m, oracle.backend_fns())
    bad, worst = [], 0.0
    for j in range(S):
        (t_h, l_h), (t_r, l_r) = s_hip.step(forced(seed, j, V), j), s_ref.step(forced(seed, j, V), j)
        worst = max(worst, check_row(f"fill {j}", l_h, l_r, t_h, t_r, tol, bad))
    assert s_hip.shift(keep, discard, S) == S - discard == 36
    cos, sin = m.rope_tables()
    c, s = M.shift_rows(cos, sin, discard)
    lanes = m.kv_lanes()
    snapshot = {l.buf: ob.buffer(s_ref.handle, l.buf).copy() for l in lanes}
    oracle_shift(ob, s_ref.handle, lanes, keep, discard, S, c, s)
    ref_rows = []
    for j in range(discard):
        pos = S - discard + j
        (t_h, l_h), (t_r, l_r) = s_hip.step(forced(seed, S + j, V), pos), s_ref.step(forced(seed, S + j, V), pos)
        worst = max(worst, check_row(f"past {pos}", l_h, l_r, t_h, t_r, tol, bad))
        ref_rows.append(l_r)
    assert not be.last_error(), be.last_error()
    print("worst:", worst)
    assert not bad, bad
    if not kvq:
        for buf, img in snapshot.items():
            ob.buffer(s_ref.handle, buf)[:] = img
        oracle_shift(ob, s_ref.handle, lanes, keep, discard, S, c, s, rotate=False)
        gap = 0.0
        for j in range(discard):
            _, l_u = s_ref.step(forced(seed, S + j, V), S - discard + j)
            gap = max(gap, float(np.abs(l_u - ref_rows[j]).max() / np.abs(ref_rows[j]).max()))
        print("control: the unrotated oracle differs by", gap)
        assert gap > 2 * tol
    s_hip.close(), s_ref.close(), m.close()


@pytest.mark.parametrize("kvq", [0, 32])
def test_one_sequence_of_a_batch_is_shifted_alone(hip_backend, oracle, kvq):
    """3 sequences on tiny64 (f32 slabs / int8 caches) step 20 forced tokens each; sequence 1 is shifted (keep 4, discard 8) while
    0 and 2 are not — their cache bytes are unchanged —, and one batched step at positions [20, 12, 20] follows against the oracle."""
    be, B, n, keep, discard = hip_backend, 3, 20, 4, 8
    cfg = tiny64()
    V = cfg.vocab_size
    tol = KVQ_TOL if kvq else F32_TOL
    bm = llama.BatchModel(cfg, B, llama.Q4_0, kv_quant_block=kvq)
    ob = oracle.OracleBackend()
    s_hip, s_ref = llama.BatchSession(bm, llama.hip_backend_fns(be), B), llama.BatchSession(bm, oracle.backend_fns(), B)
    bad = []
    for j in range(n):
        toks, pos = [forced(b + 1, j, V) for b in range(B)], [j] * B
        (t_h, l_h), (t_r, l_r) = s_hip.step(toks, pos), s_ref.step(toks, pos)
        for b in range(B):
            check_row(f"fill {j} seq {b}", l_h[b], l_r[b], t_h[b], t_r[b], tol, bad)
    bufs = sorted({l.buf for l in bm.kv_lanes()})
    size = {b: bm.program.buffer_sizes[b] for b in bufs}
    before = {b: download(be, s_hip.handle, b, size[b]) for b in bufs}
    assert s_hip.shift(1, keep, discard, n) == n - discard
    cos, sin = bm.rope_tables()
    c, s = M.shift_rows(cos, sin, discard)
    oracle_shift(ob, s_ref.handle, bm.kv_lanes(1), keep, discard, n, c, s)
    after = {b: download(be, s_hip.handle, b, size[b]) for b in bufs}
    # what may have changed: sequence 1's lanes, columns [keep, n - discard); everything else is bit-identical
    want = {b: a.copy() for b, a in before.items()}
    for i, l in enumerate(bm.kv_lanes(1)):
        if l.block_size:
            M.shift_cache_image(want[l.buf], l.n_cols, l.d_head, keep, discard, n, i % 2 == 0, c, s)
        else:
            view = want[l.buf][l.offset:l.offset + l.n_cols * l.d_head].reshape(l.n_cols, l.d_head)
            view[:] = M.shift_f32(view, keep, discard, n, i % 2 == 0, c, s)
    changed = 0
    for b in bufs:
        assert np.array_equal(after[b].view(np.uint32), want[b].view(np.uint32)), b
        changed += int(np.count_nonzero(after[b].view(np.uint32) != before[b].view(np.uint32)))
    assert changed > 0
    for seq in (0, 2):
        for l in bm.kv_lanes(seq):
            lo, hi = (0, size[l.buf]) if l.block_size else (l.offset, l.offset + l.n_cols * l.d_head)
            assert np.array_equal(after[l.buf][lo:hi].view(np.uint32), before[l.buf][lo:hi].view(np.uint32)), (seq, l.buf)
    toks, pos = [forced(b + 1, n, V) for b in range(B)], [n, n - discard, n]
    (t_h, l_h), (t_r, l_r) = s_hip.step(toks, pos), s_ref.step(toks, pos)
    for b in range(B):
        check_row(f"after the shift seq {b}", l_h[b], l_r[b], t_h[b], t_r[b], tol, bad)
    assert not be.last_error(), be.last_error()
    assert not bad, bad
    s_hip.close(), s_ref.close(), bm.close()


def test_resident_decode_from_the_shifted_position_equals_vtable_stepping(hip_backend):
    """The project's standing check of the two paths, from a shifted state: fill tiny64's cache with forced tokens, shift
    (keep 4, discard 28), then 8 tokens of the resident loop from position 36 equal 8 vtable steps from the same state."""
    be = hip_backend
    cfg = tiny64()
    S, V = cfg.max_seq_len, cfg.vocab_size
    m = llama.Model(cfg, llama.Q4_0)
    s = llama.Session(m, llama.hip_backend_fns(be))
    s.resident_setup(be)
    for j in range(S):
        s.step(forced(2, j, V), j, want_logits=False)
    pos = s.shift(4, 28, S)
    assert pos == 36
    first = forced(2, S, V)
    got = s.resident_decode(first, pos, 8)
    assert not be.last_error(), be.last_error()
    want, _ = s.decode(first, pos, 8)  # (rewrites columns 36..43 with what the resident loop wrote there)
    assert got.tolist() == want.tolist()
    s.close(), m.close()
