"""The case table of tests/generic_cases.py, pinned on the CPU before any device runs: the restated launcher rules give every case
the route the table names and every route is covered; the float64 references agree with the oracle under the oracle's own bounds
(its summation depth in the same formulas), which shows that the bounds are sound and that the inputs keep the reference inside
them; the exact claims hold on the oracle."""
from dataclasses import replace

import numpy as np
import pytest

from tests import generic_cases as GC

f32 = np.float32


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (case, [buffers per execute]) on the oracle: computed once per case, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            c = GC.nosplit_case(int(name.split("_")[1])) if name.startswith("nosplit_") else GC.build_case(name)
            cache[name] = (c, GC.run_oracle(oracle.OracleBackend(), c))
        return cache[name]
    return get


def test_rows_routes_and_coverage():
    seen = set()
    for (rows, cols), want in GC.ROW_SHAPES:
        for fused in (False, True):
            want_f = want or (("loop" if fused else "rmsnorm_kernel"), 1)
            assert GC.row_route(rows, cols, fused) == want_f, (rows, cols, fused)
            seen.add((want_f[0], want_f[1] > 1))
    # every form x {one workgroup per row, several} the launcher can produce up to 8192 columns, and both forms beyond
    assert seen == {(f, s) for f in ("npt4", "npt16", "npt32") for s in (False, True)} | {("loop", False), ("rmsnorm_kernel", False)}
    assert GC.row_route(4, 1000) == ("npt4", 4)  # the special rows
    assert GC.row_route(2, 1000)[1] * 256 - 1000 == 24  # the last chunk of the split (2, 1000) rows is 232 wide
    for cols in GC.NOSPLIT_COLS:
        assert GC.row_route(2, cols, True)[1] > 1 and GC.row_route(GC.NOSPLIT_ROWS, cols, True)[1] == 1
    for name in GC.names_of("rows"):
        c = GC.build_case(name) if "128x" not in name and "129x" not in name else None  # (the two large ones are covered by the loop above)
        assert c is None or c.route == c.want_route, name


def test_dense_and_chain_routes_and_coverage():
    dense = set()
    for name in GC.names_of("dense"):
        c = GC.build_case(name)
        assert c.route == c.want_route, name
        dense.add(c.route[0])
    assert dense == {"ncontig", "kcontig4", "kcontig1", "strided"}  # all but the streaming form (tests/test_hip_lm_head_stream.py)
    # the scalar K-contiguous kernel once for each reason, and only that reason
    base = dict(a_col_stride=1, K=64, a_row_stride=64, b_col_stride=64, a_offset=0, b_offset=0)
    broken = {"dense_kcontig1_k_mod_4": ("K", "a_row_stride", "b_col_stride"), "dense_kcontig1_a_cs": ("a_col_stride", "a_row_stride"),
              "dense_kcontig1_b_cs": ("b_col_stride",), "dense_kcontig1_a_offset": ("a_offset",)}
    for name, fields in broken.items():
        g = GC.DENSE[name][0]
        assert all(getattr(g, k) == v for k, v in base.items() if k not in fields), name
        assert GC.dense_route(replace(g, **{k: base[k] for k in fields})) == "kcontig4", name
    chains = set()
    for name in GC.names_of("chains"):
        c = GC.build_case(name) if "vec4" not in name and "unaligned" not in name else None
        if c is not None:
            assert c.route == c.want_route, name
            chains.add(c.route[0])
    assert GC.chain_route(1 << 20, True, False) == "pre4" and GC.chain_route((1 << 20) + 4, False, False) == "pre1"
    assert GC.chain_route((1 << 20) - 4, True, False) == "pre1" and GC.chain_route(1 << 20, True, True) == "step"
    assert chains | {"pre4"} == {"step", "pre1", "pre4"}


@pytest.mark.parametrize("name", GC.CASE_NAMES)
def test_oracle_within_its_bounds(runs, name):
    """every float64 reference against the oracle under the oracle's bound; the exactly rounded ops, the special values among them,
    against numpy float32 (relu by value); the in-place forms against the out-of-place ones; and nothing written outside the spans"""
    c, outs = runs(name)
    assert c.group in GC.GROUPS and name in GC.names_of(c.group) and (c.route is None or c.route == c.want_route)
    worst = 0.0
    for bufs in outs:
        for ck in c.checks:
            worst = max(worst, GC.hold(ck, bufs, "obound", oracle_bufs=bufs))
        GC.untouched(c, bufs)
    print(f"{name}: max oracle error / bound = {worst:.3g}")


def block_sum_f32(v):
    """the row kernels' summation order in float32, rows of v at once: thread t chains elements t, t + 256, ..., a 64-lane xor-shuffle
    tree folds each wave, the four wave sums are added in order (kernels_generic.hip wave_sum, block_sum)"""
    rows, cols = v.shape
    chunks = GC.cdiv(cols, 256)
    pad = np.zeros((rows, chunks * 256), f32)
    pad[:, :cols] = v
    part = np.zeros((rows, 256), f32)
    for k in range(chunks):
        part = part + pad[:, 256 * k:256 * (k + 1)]
    lane = np.arange(256)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ off]
    total = np.zeros(rows, f32)
    for w in range(4):
        total = total + part[:, 64 * w]
    return total[:, None]


@pytest.mark.parametrize("name", [n for n in GC.names_of("rows") if "specials" not in n] + [f"layernorm_{r}x{c}" for r, c in GC.SM_SHAPES])
def test_device_bounds_hold_for_the_kernels_own_order(name):
    """the a-priori bounds the device is held to (D = ceil(cols / 256)) against a float32 emulation of its kernels on the case's own
    inputs: a correct kernel fits them with room, so a miss on the device is the kernel's"""
    c = GC.build_case(name)
    rows, cols = c.info["rows"], c.info["cols"]
    colsf, eps = f32(cols), f32(GC.EPS)
    emu = {}
    if c.group == "rows":
        x = c.info["x"].reshape(rows, cols)
        h = x + c.info["y"].reshape(rows, cols) if c.info["fused"] else x
        nrm = h * (f32(1) / np.sqrt(block_sum_f32(h * h) / colsf + eps))
        emu = {"rmsnorm": nrm, "norm": nrm, "sum": h}
        if c.info["fused"]:
            emu["product"] = nrm * c.info["g"].reshape(rows, cols)
    else:
        x = c.upload(0)[GC.SO:].reshape(rows, cols)
        d = x - block_sum_f32(x) / colsf
        emu = {"layernorm": d * (f32(1) / np.sqrt(block_sum_f32(d * d) / colsf + eps))}
    worst = 0.0
    for ck in c.checks:
        if ck.what in emu:
            bufs = {ck.buf: np.zeros(c.prog.buffer_sizes[ck.buf], f32)}
            bufs[ck.buf][ck.idx] = emu[ck.what].astype(f32).ravel()
            worst = max(worst, GC.hold(ck, bufs, "bound"))
    print(f"{name}: max emulated error / bound = {worst:.3g}")


@pytest.mark.parametrize("cols", GC.NOSPLIT_COLS)
def test_nosplit_rows_are_the_split_rows(runs, cols):
    c, (bufs,) = runs(f"nosplit_{cols}")
    small, (sbufs,) = runs(f"chain_2x{cols}")
    assert c.route == ("npt4" if cols <= 1024 else "npt16" if cols <= 4096 else "npt32", 1) and small.route[1] > 1
    for ck in c.checks:
        GC.hold(ck, bufs, "obound")
    for buf, idx, sbuf, sidx in c.info["pairs"]:
        assert GC.same_bits(bufs[buf][idx], sbufs[sbuf][sidx])


def test_exact_claims_on_the_oracle(runs):
    c, (bufs,) = runs("softmax_specials")
    out = bufs[c.checks[0].buf][c.checks[0].idx].reshape(5, 300)
    x = c.upload(0)[GC.SO:].reshape(5, 300)
    assert out[0, 17] == 1 and np.count_nonzero(out[0]) == 1          # all -inf but one element
    assert np.all(out[3] == 0)                                         # one +inf: the finite-shift guard zeroes the row
    assert out[4, 257] == 0 and abs(float(out[4].sum()) - 1) < 1e-5    # the max ignores the NaN, which comes out 0
    assert np.all(out[2][np.abs(x[2]) < 1e29] == 0) and np.all(out[2][x[2] == -1e30] == 0)
    c, (bufs,) = runs("layernorm_specials")
    assert np.all(bufs[c.checks[0].buf][c.checks[0].idx][:300] == 0)   # the constant row
    c, (bufs,) = runs("reduce_specials")
    mx = bufs[c.checks[1].buf][c.checks[1].idx]
    x = c.upload(0)[GC.SO:].reshape(3, 130)
    assert mx[0] == -np.inf and mx[1] == np.nanmax(x[1]) and mx[2] == 1e8
    for name in ("rows_specials_rmsnorm", "rows_specials_chain"):
        c, (bufs,) = runs(name)
        for ck in c.checks:
            if ck.mode == "bound" and ck.what != "sum":
                assert np.all(bufs[ck.buf][ck.idx][:1000] == 0), name  # the all-zero row


@pytest.mark.parametrize("op", GC.EXACT_OPS + ("relu",))
def test_special_values_through_the_oracle(runs, op):
    c, (bufs,) = runs("elt_" + op)
    ck = c.checks[-1]
    assert ck.mode == ("value" if op == "relu" else "bits") and ck.idx.size == (225 if op in ("add", "mul") else 15)
    GC.hold(ck, bufs)
