"""zgml_hip_kv_move on the MI355X (zgml_amd/csrc/kv_move.hip): KV columns of many lanes from one compiled program to another in
one launch. Bit contracts: f32 -> f32 and int8 -> int8 are copies (every other byte of every touched buffer keeps its pattern);
f32 -> int8 writes what a GPU program of kvq_store ops writes for the same columns (device against device, to the bit; against the
oracle within one quantisation unit per value and 1 ulp per scale); a fork inside one batched plan; every refusal returns -1 with a
text and leaves nothing sticky; and the admission of prefilled prompts into an int8 batched plan end to end against the oracle."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, capi, llama
from zgml_amd.program import ios_to_c
from tests.kvq_cases import check_against_trace, oracle_trace, tiny64

pytestmark = pytest.mark.gpu
f32 = np.float32
PATTERN = 0xA5


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


def kv_move(be, dst, dst_lanes, src, src_lanes, src_col, dst_col, n):
    return capi.load_hip().zgml_hip_kv_move(be.ctx, dst, lanes_c(dst_lanes), src, lanes_c(src_lanes), len(dst_lanes), src_col, dst_col, n)


def pattern(n_elems):
    return np.full(n_elems * 4, PATTERN, np.uint8).view(f32)


def rand_cols(rng, n_cols, dh):
    c = ((rng.random((n_cols, dh)) - 0.5) * 2).astype(f32)
    c[1 % n_cols, :32] = 0.0  # an all-zero block
    return c


def rand_cache(rng, n_cols, dh):
    """a quantised cache image with arbitrary bytes and scales"""
    img = np.zeros(cache_elems(n_cols, dh), f32)
    img[:n_cols * dh // 4] = rng.integers(0, 2 ** 32, n_cols * dh // 4, dtype=np.uint64).astype(np.uint32).view(f32)
    img[n_cols * dh // 4:] = rng.random(n_cols * (dh // 32)).astype(f32) + f32(0.01)
    return img


CASES = [(3, 5, 1), (3, 5, 7), (3, 5, 33), (0, 0, None)]  # (src_col, dst_col, n); None: n = n_cols


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_f32_to_f32_copies_columns_and_nothing_else(hip_backend, dh):
    """Two lanes per call: one 16-byte aligned on both sides, one at an odd f32 offset (the dword path); the destination has a
    different n_cols and lane offset than the source."""
    be, rng = hip_backend, np.random.default_rng(dh)
    n_src, n_dst = 48, 56
    src_off, dst_off = [0, 3 + 48 * dh], [8, 8 + 56 * dh + 1]
    src_img = ((rng.random(src_off[1] + n_src * dh + 5) - 0.5) * 2).astype(f32)
    n_dst_elems = dst_off[1] + n_dst * dh + 7
    hs = holder(be, [src_img.size], {0: src_img})
    for src_col, dst_col, n in CASES:
        n = n or n_src
        hd = holder(be, [n_dst_elems], {0: pattern(n_dst_elems)})
        rc = kv_move(be, hd, [(0, o, dh, n_dst, 0) for o in dst_off], hs, [(0, o, dh, n_src, 0) for o in src_off], src_col, dst_col, n)
        assert rc == 0 and not be.last_error(), be.last_error()
        got = download(be, hd, 0, n_dst_elems)
        want = pattern(n_dst_elems)
        for so, do in zip(src_off, dst_off):
            want[do + dst_col * dh:do + (dst_col + n) * dh] = src_img[so + src_col * dh:so + (src_col + n) * dh]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (src_col, dst_col, n)
        be.freeProgram(hd)
    be.freeProgram(hs)


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_int8_to_int8_copies_bytes_and_scales_and_nothing_else(hip_backend, dh):
    be, rng = hip_backend, np.random.default_rng(100 + dh)
    n_src, n_dst, bpc = 48, 56, dh // 32
    imgs = [rand_cache(rng, n_src, dh) for _ in range(2)]
    hs = holder(be, [i.size for i in imgs], dict(enumerate(imgs)))
    ce_d = cache_elems(n_dst, dh) + 3  # (three more floats than the cache needs: they keep their pattern too)
    for src_col, dst_col, n in CASES:
        n = n or n_src
        hd = holder(be, [ce_d, ce_d], {0: pattern(ce_d), 1: pattern(ce_d)})
        rc = kv_move(be, hd, [(b, 0, dh, n_dst, 32) for b in (0, 1)], hs, [(b, 0, dh, n_src, 32) for b in (0, 1)], src_col, dst_col, n)
        assert rc == 0 and not be.last_error(), be.last_error()
        for b in (0, 1):
            got = download(be, hd, b, ce_d)
            want = pattern(ce_d)
            wb, sb = want.view(np.uint8), imgs[b].view(np.uint8)
            wb[dst_col * dh:(dst_col + n) * dh] = sb[src_col * dh:(src_col + n) * dh]
            s_sc, d_sc = n_src * dh // 4, n_dst * dh // 4
            want[d_sc + dst_col * bpc:d_sc + (dst_col + n) * bpc] = imgs[b][s_sc + src_col * bpc:s_sc + (src_col + n) * bpc]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (src_col, dst_col, n, b)
        be.freeProgram(hd)
    be.freeProgram(hs)


@pytest.mark.parametrize("dh", [32, 64, 128, 256])
def test_f32_to_int8_equals_kvq_store_on_the_device(hip_backend, oracle, dh):
    """The moved columns' bytes and scales are, to the bit, what kvq_store ops write for the same f32 columns into an equally sized
    cache on the GPU; against the oracle's kvq_store: one quantisation unit per value, 1 ulp per scale. Two source lanes: aligned,
    and at an odd f32 offset (scalar loads)."""
    be, rng = hip_backend, np.random.default_rng(200 + dh)
    n_src, n_dst, bpc = 40, 48, dh // 32
    src_off = [0, n_src * dh + 1]
    cols = [rand_cols(rng, n_src, dh) for _ in src_off]
    cols[0][2] *= f32(1e-30)  # tiny magnitudes
    cols[1][4, 5], cols[1][4, 9] = 3.0, -3.0
    src_img = np.zeros(src_off[1] + n_src * dh, f32)
    for o, c in zip(src_off, cols):
        src_img[o:o + n_src * dh] = c.ravel()
    hs = holder(be, [src_img.size], {0: src_img})
    ce = cache_elems(n_dst, dh)
    for src_col, dst_col, n in CASES:
        n = n or n_src
        hd = holder(be, [ce, ce], {0: pattern(ce), 1: pattern(ce)})
        rc = kv_move(be, hd, [(b, 0, dh, n_dst, 32) for b in (0, 1)], hs, [(0, o, dh, n_src, 0) for o in src_off], src_col, dst_col, n)
        assert rc == 0 and not be.last_error(), be.last_error()
        for b in (0, 1):
            got = download(be, hd, b, ce)
            # the same columns through kvq_store ops into a cache of the same size, pre-filled with the same pattern
            moved = np.ascontiguousarray(cols[b][src_col:src_col + n])
            prog = DeviceProgram(ops=[DeviceOp.kvq_store(0, 1, dh, 32, n_dst, c * dh, 0, dst_col + c, 1) for c in range(n)], buffer_sizes=[ce, n * dh],
                                 initial_uploads=[ProgramIO(0, pattern(ce)), ProgramIO(1, moved.ravel())])
            outs = []
            for backend in (be, oracle.OracleBackend()):
                h = backend.compileProgram(prog)
                out = np.zeros(ce, f32)
                backend.executeProgram(h, [], [ProgramIO(0, out)])
                backend.freeProgram(h)
                outs.append(out)
            assert np.array_equal(got.view(np.uint32), outs[0].view(np.uint32)), (src_col, dst_col, n, b)
            nq = n_dst * dh // 4
            dq = got[:nq].view(np.int8).astype(np.int32) - outs[1][:nq].view(np.int8).astype(np.int32)
            assert np.abs(dq).max() <= 1
            ds = got[nq:].view(np.int32).astype(np.int64) - outs[1][nq:].view(np.int32).astype(np.int64)
            assert np.abs(ds).max() <= 1
        be.freeProgram(hd)
    be.freeProgram(hs)


def test_f32_to_int8_zero_in_a_tiny_block_follows_the_reference(hip_backend, oracle):
    """The one input on which the move and the device's kvq_store differ (zgml_amd/csrc/kvq.h): a block whose largest magnitude is
    below 127 / FLT_MAX has inv = +inf, an exact zero in it gives NaN, and the reference's clamp makes that 127. Against the oracle's
    kvq_store: the bytes equal, the scales within 1 ulp."""
    be, dh, nc = hip_backend, 64, 4
    cols = np.zeros((nc, dh), f32)
    cols[0, :32] = np.where(np.arange(32) % 3 == 0, 0.0, 2e-38).astype(f32) * np.where(np.arange(32) % 2, 1, -1).astype(f32)
    cols[0, 32:] = np.linspace(-1, 1, 32).astype(f32)
    cols[1, :] = f32(3e-38)
    cols[1, 7] = 0.0
    cols[2:] = np.random.default_rng(9).random((2, dh)).astype(f32)
    ce = cache_elems(nc, dh)
    hs, hd = holder(be, [nc * dh], {0: cols.ravel()}), holder(be, [ce], {0: pattern(ce)})
    assert kv_move(be, hd, [(0, 0, dh, nc, 32)], hs, [(0, 0, dh, nc, 0)], 0, 0, nc) == 0 and not be.last_error(), be.last_error()
    got = download(be, hd, 0, ce)
    prog = DeviceProgram(ops=[DeviceOp.kvq_store(0, 1, dh, 32, nc, c * dh, 0, c, 1) for c in range(nc)], buffer_sizes=[ce, nc * dh],
                         initial_uploads=[ProgramIO(1, cols.ravel())])
    want = oracle.run_program(prog, 0, ce)
    nq = nc * dh // 4
    gq, wq = got[:nq].view(np.int8).reshape(nc, dh), want[:nq].view(np.int8).reshape(nc, dh)
    assert wq[0, 0] == 127 and wq[1, 7] == 127  # (the corner is in the data: the reference's byte for 0 * inf)
    assert np.array_equal(gq, wq)
    assert np.abs(got[nq:].view(np.int32).astype(np.int64) - want[nq:].view(np.int32).astype(np.int64)).max() <= 1
    be.freeProgram(hs), be.freeProgram(hd)


@pytest.mark.parametrize("kvq", [0, 32])
def test_fork_inside_one_batched_plan(hip_backend, kvq):
    be, B, n = hip_backend, 3, 11
    bm = llama.BatchModel(tiny64(), B, llama.Q4_0, kv_quant_block=kvq)
    s = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    toks, pos = np.array([3, 40, 77]), np.zeros(B, np.int64)
    for _ in range(n):  # every sequence fills its own first n columns
        toks, _ = s.step(toks, pos)
        pos += 1
    bufs = sorted({l.buf for l in bm.kv_lanes()})
    size = {b: bm.program.buffer_sizes[b] for b in bufs}
    before = {b: download(be, s.handle, b, size[b]) for b in bufs}
    s.fork(0, 2, n)
    be.synchronize()
    assert not be.last_error(), be.last_error()
    after = {b: download(be, s.handle, b, size[b]) for b in bufs}
    want = {b: a.copy() for b, a in before.items()}
    for ls, ld in zip(bm.kv_lanes(0), bm.kv_lanes(2)):
        dh = ls.d_head
        if kvq:
            wb, sb, sc = want[ld.buf].view(np.uint8), before[ls.buf].view(np.uint8), ls.n_cols * dh // 4
            wb[:n * dh] = sb[:n * dh]
            want[ld.buf][sc:sc + n * dh // 32] = before[ls.buf][sc:sc + n * dh // 32]
        else:
            want[ld.buf][ld.offset:ld.offset + n * dh] = before[ls.buf][ls.offset:ls.offset + n * dh]
    changed = 0
    for b in bufs:
        assert np.array_equal(after[b].view(np.uint32), want[b].view(np.uint32)), b
        changed += int(np.count_nonzero(after[b].view(np.uint32) != before[b].view(np.uint32)))
    assert changed > 0  # (sequences 0 and 2 decoded different tokens: the fork moved something)
    # the forked sequence continues exactly as its source does from here
    t, l = s.step([int(toks[0]), int(toks[1]), int(toks[0])], [n, n, n])
    assert np.array_equal(l[0], l[2]) and t[0] == t[2]
    with pytest.raises(ValueError):
        s.fork(1, 1, n)
    s.close(), bm.close()


def test_refusals_leave_nothing_sticky(hip_backend):
    be, hip = hip_backend, capi.load_hip()
    dh, nc = 64, 16
    ce = cache_elems(nc, dh)
    # buffers: 0 f32 slab (two lanes' worth), 1 / 2 int8 caches, 3 an f32 slab, 4 dead (no op references it)
    sizes = [2 * nc * dh, ce, ce, nc * dh]
    n = len(sizes)
    prog = DeviceProgram(ops=[DeviceOp.elementwise("add", n + 1, i, i, 1) for i in range(n)], buffer_sizes=sizes + [nc * dh, 1])
    h = be.compileProgram(prog)
    F, Q = (0, 0, dh, nc, 0), (1, 0, dh, nc, 32)
    bad = [
        ("dead", [(4, 0, dh, nc, 0)], [F], 0, 0, 4),                       # a dead (elided) destination buffer
        ("dead", [F], [(4, 0, dh, nc, 0)], 0, 0, 4),                       # ... source buffer
        ("no such", [(9, 0, dh, nc, 0)], [F], 0, 0, 4),                    # a buffer id outside the program
        ("d_head", [(3, 0, 32, 2 * nc, 0)], [F], 0, 0, 4),                 # d_head mismatch
        ("n_cols", [(3, 0, dh, nc, 0)], [F], 0, 13, 4),                    # columns beyond the destination's n_cols
        ("n_cols", [(3, 0, dh, nc, 0)], [F], 14, 0, 4),                    # ... the source's
        ("n_cols", [(3, 0, dh, nc, 0)], [F], 0xFFFFFFFF, 0, 2),            # (col + n wraps in 32 bits)
        ("extent", [(3, 1, dh, nc, 0)], [F], 0, 0, 4),                     # an f32 lane that ends past its buffer
        ("extent", [(1, 0, dh, nc + 1, 32)], [F], 0, 0, 4),                # an int8 lane larger than its buffer
        ("block_size", [(1, 0, dh, nc, 16)], [F], 0, 0, 4),                # block size other than 0 / 32
        ("d_head % 32", [(1, 0, 48, nc, 32)], [(0, 0, 48, nc, 0)], 0, 0, 4),
        ("offset", [(1, 4, dh, nc - 1, 32)], [F], 0, 0, 4),                # an int8 lane with an offset
        ("int8 -> f32", [(3, 0, dh, nc, 0)], [Q], 0, 0, 4),
        ("overlapping", [F], [F], 0, 2, 4),                                # a lane pair that overlaps itself
        ("overlapping", [Q], [Q], 3, 0, 4),
        ("overlapping", [(0, nc * dh, dh, nc, 0), (3, 0, dh, nc, 0)], [F, (0, nc * dh, dh, nc, 0)], 0, 0, 4),  # pair 1 reads what pair 0 writes
    ]
    for word, dl, sl, sc, dc, cnt in bad:
        assert kv_move(be, h, dl, h, sl, sc, dc, cnt) == -1, word
        err = be.last_error()
        assert err.startswith("kv_move") and word in err, (word, err)
        hip.zgml_hip_clear_error(be.ctx)
    # nothing to do: 0 and no error, whatever the lanes say
    assert kv_move(be, h, [], h, [], 0, 0, 4) == 0 and kv_move(be, h, [(9, 0, dh, nc, 7)], h, [F], 0, 0, 0) == 0
    assert not be.last_error()
    # a valid call still works: same-buffer move between disjoint column ranges, and f32 -> int8
    assert kv_move(be, h, [F, Q], h, [F, (0, nc * dh, dh, nc, 0)], 0, 8, 4) == 0
    be.synchronize()
    assert not be.last_error(), be.last_error()
    be.freeProgram(h)


def test_admission_end_to_end_matches_the_oracle(hip_backend, oracle):
    """Prompts of 4, 6 and 8 tokens are prefilled on f32 T-token plans, admitted into slots 0..2 of an int8 batched plan (one
    kv_move launch each: quantised on the way) and decoded for 3 batched steps; the oracle does the same with its hand-over done
    by kvq_store ops over the prefill plan's f32 columns. Bound: that of the int8 caches (tests/kvq_cases.py)."""
    be, B, cfg = hip_backend, 3, tiny64()
    fns_h, fns_o, ob = llama.hip_backend_fns(be), oracle.backend_fns(), oracle.OracleBackend()
    base = llama.Model(cfg, llama.Q4_0)
    bm = llama.BatchModel(cfg, B, like=base, kv_quant_block=32)
    s_hip, s_ref = llama.BatchSession(bm, fns_h, B), llama.BatchSession(bm, fns_o, B)
    dh, S = cfg.d_head, cfg.max_seq_len
    toks, pos = [], []
    for b in range(B):
        T = 4 + 2 * b
        prompt = [(49 * (b + 1) + 5 * j + 1) % cfg.vocab_size for j in range(T)]  # (prompts after which the oracle's three rows are decisive)
        mp = llama.Model(cfg, llama.Q4_0, token_len=T)
        ph, po = llama.Session(mp, fns_h), llama.Session(mp, fns_o)
        t_h, l_h = ph.prefill(prompt, 0)
        t_o, l_o = po.prefill(prompt, 0)
        assert np.abs(l_h - l_o).max() <= 2e-4 * np.abs(l_o).max()  # (the f32 plans' bound, tests/test_hip_llama.py)
        s_hip.admit(b, ph, T)
        # the oracle's hand-over: every f32 lane's first T columns through kvq_store ops into the slot's cache
        for ls, ld in zip(mp.kv_lanes(), bm.kv_lanes(b)):
            cols = ob.buffer(po.handle, ls.buf)[ls.offset:ls.offset + T * dh].copy()
            ce = cache_elems(S, dh)
            prog = DeviceProgram(ops=[DeviceOp.kvq_store(0, 1, dh, 32, S, c * dh, 0, c, 1) for c in range(T)], buffer_sizes=[ce, T * dh],
                                 initial_uploads=[ProgramIO(1, cols)])
            ob.buffer(s_ref.handle, ld.buf)[:ce] = oracle.run_program(prog, 0, ce)
        toks.append(t_o), pos.append(T)
        be.synchronize()  # (the move has read the prefill plan's caches before the plan is freed)
        ph.close(), po.close(), mp.close()
    assert not be.last_error(), be.last_error()
    trace = oracle_trace(s_ref, toks, pos, 3)
    print("worst, decisive, rows:", check_against_trace(be, s_hip, trace))
    s_hip.close(), s_ref.close(), bm.close(), base.close()
