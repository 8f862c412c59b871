"""The streaming form of the M = 1, K-contiguous f32 dense matmul (the tied LM head: kernels_generic.hip,
dense_kcontig_stream_kernel), and the resident greedy loop's token tail that rides on it (runtime_resident.hip: the head leaves
the argmax pairs and the position part of the next step's prep, stage 2 copies the embedding row).

The rows: the streaming form keeps the arithmetic of dense_kcontig_kernel<float, 4> — the same fmaf chain per lane, the same wave
fold — and changes only the schedule, so its result is held to the BITS of the old kernel's. The old kernel is reached with the same
data as an M = 2 program whose two A rows are equal (M > 1 never takes the streaming form): row 0 of that result, viewed as uint32,
must equal the M = 1 result. A K above the unroll bound (1024) and a B base off the 16-byte grid take the old kernel at M = 1
too and must agree all the same. Rows per workgroup: 4 waves of 2 rows = 8; at most 1024 workgroups take the rows, so more than
8192 rows are strided over (N = 8203: two workgroups take a second block, the last one short).

The pairs: with a tied head, equal embedding rows give logits equal to the bit, so duplicated rows are exact ties. The loop must
return the LOWEST index of the tie (first maximum wins, as the host-side argmax of vtable stepping does), wherever the tied rows
lie among the head's workgroups, and its tokens must equal those of vtable stepping.

The loop's edges: a call at pos > 0, a resumed call, a call that ends at the context's last position followed by one at position
0, calls of one and of no step, and resident / vtable / resident on one session."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, MatMulGeometry, ProgramIO, llama

pytestmark = pytest.mark.gpu
f32 = np.float32
WG_ROWS = 8       # rows a workgroup of the streaming form produces
MAX_WGS = 1024    # workgroups that take the rows: beyond MAX_WGS * WG_ROWS rows they stride
UNROLL_K = 1024   # the largest K it takes


def _run(be, prog, idx, n):
    h = be.compileProgram(prog)
    assert h, be.last_error()
    out = np.zeros(n, f32)
    try:
        be.executeProgram(h, [], [ProgramIO(idx, out)])
    finally:
        be.freeProgram(h)
    assert not be.last_error(), be.last_error()
    return out


def _head(be, x, w, M, b_off=0):
    """x [K] and w [N][K] (B K-contiguous: b_row_stride 1, b_col_stride K) as an M-row program, every A row = x -> [M][N]"""
    N, K = w.shape
    a = np.tile(x, M).astype(f32)
    b = np.concatenate([np.full(b_off, 3, f32), w.ravel()])
    g = MatMulGeometry(M=M, N=N, K=K, a_row_stride=K, a_col_stride=1, b_row_stride=1, b_col_stride=K,
                       a_offset=0, b_offset=b_off, dst_offset=0, dst_row_stride=N)
    prog = DeviceProgram(ops=[DeviceOp.matmul(2, 0, 1, g)], buffer_sizes=[a.size, b.size, M * N + 1],
                         initial_uploads=[ProgramIO(0, a), ProgramIO(1, b), ProgramIO(2, np.full(M * N + 1, -7, f32))])
    out = _run(be, prog, 2, M * N + 1)
    assert out[M * N] == -7  # nothing written past the rows
    return out[:M * N].reshape(M, N)


def _same_bits(be, x, w, b_off=0):
    got = _head(be, x, w, 1, b_off)[0]
    old = _head(be, x, w, 2, b_off)
    assert np.array_equal(old[0].view(np.uint32), old[1].view(np.uint32))
    assert np.array_equal(got.view(np.uint32), old[0].view(np.uint32)), (w.shape, b_off, int(np.sum(got.view(np.uint32) != old[0].view(np.uint32))))
    return got


NS = [1, 3, 1000, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1]


def test_rows_beyond_one_pass_are_strided_over(hip_backend):
    rng = np.random.default_rng(3)
    K, N = 60, MAX_WGS * WG_ROWS + WG_ROWS + 3
    _same_bits(hip_backend, rng.standard_normal(K).astype(f32), (rng.standard_normal((N, K)) * 0.05).astype(f32))


@pytest.mark.parametrize("K", [4, 60, 256, 260, 576, 1024, UNROLL_K + 4])
def test_streaming_head_equals_the_old_kernel_to_the_bit(hip_backend, K):
    rng = np.random.default_rng(K)
    for N in NS:
        x = rng.standard_normal(K).astype(f32)
        w = (rng.standard_normal((N, K)) * 0.05).astype(f32)
        got = _same_bits(hip_backend, x, w)
        # (and it is the product it claims to be. A lane chains at most 4 * ceil(K / 256) <= 20 fmaf, the wave fold adds 6 levels:
        # <= 26 roundings of 2^-24 each, 1.6e-6 of sum |x w|; 1e-5 leaves room for the float64 reference's own inputs only)
        want = w.astype(np.float64) @ x.astype(np.float64)
        bound = np.abs(w.astype(np.float64)) @ np.abs(x.astype(np.float64))
        assert np.all(np.abs(got - want) <= 1e-5 * bound + 1e-30), (K, N)


@pytest.mark.parametrize("where", ["both", "x", "b"])
def test_clamped_loads_do_not_leak_into_dead_lanes(hip_backend, where):
    """K = 260: the second k iteration is live in lane 0 alone, every other lane reads x[0] and B[row][0] again; N = 9: the rows
    past the last read B's last row. inf in exactly those places must stay where the old kernel has it."""
    K, N = 260, WG_ROWS + 1
    rng = np.random.default_rng(7)
    x = rng.standard_normal(K).astype(f32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(f32)
    if where in ("both", "x"):
        x[0] = np.inf
    if where in ("both", "b"):
        w[N - 1, 0] = np.inf
    got = _same_bits(hip_backend, x, w)
    if where == "b":  # only the last row holds the inf
        assert np.isfinite(got[:N - 1]).all() and np.isinf(got[N - 1])


def test_unaligned_b_takes_the_old_route(hip_backend):
    rng = np.random.default_rng(11)
    for N in (3, WG_ROWS + 1):
        x = rng.standard_normal(576).astype(f32)
        w = (rng.standard_normal((N, 576)) * 0.05).astype(f32)
        _same_bits(hip_backend, x, w, b_off=1)


# ── the pairs and the loop ─────────────────────────────────────────────────

def _cfg(name):
    if name == "tiny":
        return llama.preset("tiny", 64)  # vocab 512: 64 workgroups of the head
    cfg = llama.preset("smollm-135m", 64)
    cfg.n_layers, cfg.vocab_size = 1, MAX_WGS * WG_ROWS + 12  # 1026 row blocks on 1024 workgroups: two take a second block, the last of them 4 rows
    return cfg


def _plant(m, dup):
    """rows `dup` of the embedding (= the tied head) all equal one row, every other row its negated half: two tie classes"""
    e = m.token_embed()
    base = e[1].copy()
    e[:] = -0.5 * base
    e[list(dup)] = base
    return e


@pytest.mark.parametrize("name", ["tiny", "smollm-1layer"])
@pytest.mark.parametrize("dup", ["first_and_last", "two_workgroups", "inner_and_last", "all"])
def test_ties_across_workgroups_return_the_lowest_index(hip_backend, name, dup):
    cfg = _cfg(name)
    V = cfg.vocab_size
    rows = {"first_and_last": [0, V - 1], "two_workgroups": [WG_ROWS + 1, 2 * WG_ROWS + 8, V - 2], "inner_and_last": [5, V - 1],
            "all": list(range(V))}[dup]
    m = llama.Model(cfg, llama.Q4_0, threads=8)
    _plant(m, rows)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    try:
        s.resident_setup(hip_backend)
        got = s.resident_decode(rows[0], 0, 24)
        assert not hip_backend.last_error(), hip_backend.last_error()
        want, _ = s.decode(rows[0], 0, 24)
        assert got.tolist() == want.tolist()
        lowest = {min(rows)} | ({min(set(range(min(V, 8))) - set(rows))} if dup != "all" else set())
        assert set(got.tolist()) <= lowest, (got.tolist(), lowest)  # the lowest index of either tie class, nothing else
    finally:
        s.close()
        m.close()


def test_loop_edges(hip_backend):
    max_seq = 64
    m = llama.Model(llama.preset("tiny", max_seq), llama.Q4_0, threads=8)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    ok = lambda: not hip_backend.last_error()
    try:
        want = s.decode(5, 0, max_seq)[0].tolist()  # vtable stepping over the whole context (and a warm cache everywhere)
        s.resident_setup(hip_backend)
        assert s.resident_decode(want[9], 10, 5).tolist() == want[10:15] and ok()        # a call at pos > 0
        a = s.resident_decode(5, 0, 12).tolist()
        b = s.resident_decode(a[11], 12, 12).tolist()                                    # resumed
        assert a + b == want[:24] and ok()
        c = s.resident_decode(want[max_seq - 7], max_seq - 6, 6).tolist()                # ends at the last position ...
        assert c == want[max_seq - 6:] and ok()
        assert s.resident_decode(5, 0, 8).tolist() == want[:8] and ok()                  # ... then a call at position 0
        assert s.resident_decode(5, 0, 1).tolist() == want[:1] and ok()                  # one step
        assert s.resident_decode(5, 0, 0).tolist() == [] and ok()                        # no step
        assert s.resident_decode(want[max_seq - 2], max_seq - 1, 1).tolist() == want[max_seq - 1:] and ok()
        # resident, vtable, resident on one session
        assert s.resident_decode(5, 0, 6).tolist() == want[:6] and ok()
        for pos in range(6, 10):
            assert s.step(want[pos - 1], pos, want_logits=False)[0] == want[pos] and ok()
        assert s.resident_decode(want[9], 10, 6).tolist() == want[10:16] and ok()
    finally:
        s.close()
        m.close()
