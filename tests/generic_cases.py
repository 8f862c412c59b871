"""Named cases for the generic kernels (zgml_amd/csrc/kernels_generic.hip: elementwise ops and chains, softmax, layernorm, rmsnorm
and the [add ->] rmsnorm [-> mul] row chain, reduce, repeat, rope / slice_assign, the dense f32 matmul): the smallest shape on
each side of every launcher cut. tests/test_generic_cases_host.py pins the table on the CPU (routes, float64 references against
the oracle, the exact claims), tests/test_hip_generic_routes.py runs it on the device.

A case is a DeviceProgram plus the `Check`s of the buffers its ops write. Every destination is uploaded as -7 sentinels and is 2
elements longer than what the ops write; sources sit at offset 3 and destinations at offset 2 unless a route needs alignment, so
whatever an op must not touch is compared bit for bit with its upload. Inputs are standard_normal * 3 in f32 from a generator
seeded by the case's name.

The launcher rules the shapes were chosen by are restated here (row_route, dense_route, chain_route), each with the lines it
restates; buffers start on 256-byte boundaries (runtime.hip: "one arena for all live buffers, 256-byte aligned slots"), so a
pointer's alignment is its offset's.

Error bounds are a priori, from the kernels' operation counts, with u = 2^-24 and D = ceil(len / lanes) the number of terms one
thread chains (lanes: 256 for the row kernels, 64 for reduce and the scalar K-contiguous matmul). The oracle sums sequentially
(D = len) or in 8 lanes (rmsnorm: D = len / 8 + 8); the host test holds it to the same formulas with its own D.

  rmsnorm / row chain   |got - want| <= (D + 16) u |want|. The sum of squares has no cancellation: one square, D - 1 adds, 6 shuffle
                        levels and 3 wave adds give it (D + 10) u relative; the square root halves that; the division by cols, + eps,
                        the square root, the reciprocal and the product add 5 u: (D / 2 + 10) u in all. In the chain every input
                        of the norm carries the add's u: 2 u on the sum of squares (1 u behind the root) and 1 u on the element,
                        (D / 2 + 12) u <= (D + 16) u. The product adds one rounding: (D + 18) u.
  reduce sum            (D + 6) u sum|x| (D - 1 adds and 6 shuffle levels, each at most u times the absolute sum); max: equal bits.
  layernorm             dmu = (D + 11) u mean|x| is the error of the mean (D - 1 adds, 6 levels, 3 wave adds, the division);
                        with d = x - mean, var = mean(d^2): rel_v = (D + 12) u + (2 dmu sum|d| + cols dmu^2) / sum d^2 is the
                        relative error of the variance (its own summation plus the shifted mean), rel_i = rel_v var / (var + eps) / 2
                        + 3 u that of 1 / sqrt(var + eps), and |got - want| <= inv_std (dmu + u |d_j|) + |want_j| (rel_i + u).
  softmax               (2e-6 + (D + 12) u) want + 1e-30: 2e-6 is the relative bar the project holds the device's expf to
                        (tests/test_hip_conformance.py test_elementwise_all_ops_and_fused_chain), the subtraction of the max, the
                        positive sum, the reciprocal and the product give the rest.
  dense matmul          c u sum_k |a| |b| with c = K for one sequential fmaf chain (ncontig, strided), D + 6 for the scalar
                        K-contiguous kernel (D fmafs, 6 shuffle levels), 4 ceil(K / 256) + 6 for the four-wide one — the reasoning of
                        tests/test_hip_lm_head_stream.py. The oracle multiplies and adds apart: c = K + 1.
  elementwise           add, mul, neg, abs, sgn, step, sqrt, recip and chains of them: equal bits with numpy float32, NaN where numpy
                        has NaN (the build has -ffp-contract=off and no fast-math: correctly rounded). relu: equal values (the sign of
                        max(-0, +0) is not specified). exp, log, gelu: rtol 2e-6, atol 1e-6 against float64, the project's bar.
  repeat, rope, slice_assign   equal bits with the oracle.

gelu inputs stay in [-8, 8] (its special-value vector keeps only the members inside that range, and NaN): the reference's vector
body computes tanh as (e^2k - 1) / (e^2k + 1), which is NaN from about a > 10 on, where the device's tanhf form returns a. A known
divergence from an overflow of the reference, not something these cases test."""
import zlib
from dataclasses import dataclass, field

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, FusedEwStep, MatMulGeometry, ProgramIO

f32, f64 = np.float32, np.float64
SENTINEL = f32(-7)
U = 2.0 ** -24
PAD = 2            # a destination is this much longer than what is written into it
SO, DO = 3, 2      # source / destination offsets unless a route needs alignment
EPS = 1e-5
K_ELT, K_RMS, K_REPEAT, K_MOVE, K_FUSED = 0, 5, 7, 8, 11  # DeviceOp kinds as the plan text prints them
FLT_MIN, FLT_MAX = float(np.finfo(f32).tiny), float(np.finfo(f32).max)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.4e-45, -1.4e-45, 1e-39, -1e-39, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, 1.0, -1.0], f32)


@dataclass
class Check:
    """what one buffer must hold at `idx` after the program ran; everything outside the idx of a buffer's checks keeps the upload.
    mode "bound": |got - want| <= bound (`obound` for the oracle) against float64 `want`, non-finite `want` met exactly, `exact` (a
    mask over idx) met exactly; "bits" / "value": float32 `want` as equal bits / equal values, NaN where it has NaN; "oracle":
    equal bits with the oracle's buffer; "same": equal bits with `same` = (buffer, idx) of the same run."""
    buf: int
    idx: np.ndarray
    want: np.ndarray = None
    bound: np.ndarray = None
    obound: np.ndarray = None
    mode: str = "bound"
    exact: np.ndarray = None
    same: tuple = None
    what: str = ""


@dataclass
class Case:
    name: str
    group: str
    prog: DeviceProgram
    checks: list
    launches: tuple = ()          # (kind, n_ops, lo, hi) the plan text must show
    route: tuple = None           # what the restated launcher rule gives for the case
    want_route: tuple = None      # what the table says it must give
    refresh: tuple = ()           # move: [ops] per further execute
    inputs: tuple = ()            # repeat: ProgramIOs of a second execute
    launches_after: tuple = ()    # the plan text after that second execute
    info: dict = field(default_factory=dict)

    def upload(self, buf):
        return next(u.host for u in self.prog.initial_uploads if u.buf_idx == buf)

    def checked_buffers(self):
        return sorted({c.buf for c in self.checks})


class _B:
    def __init__(self, name):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.sizes, self.ups = [], []

    def up(self, arr):
        arr = np.ascontiguousarray(arr, dtype=f32)
        self.sizes.append(arr.size)
        self.ups.append(ProgramIO(len(self.sizes) - 1, arr))
        return len(self.sizes) - 1

    def randn(self, n):
        return (self.rng.standard_normal(n) * 3).astype(f32)

    def src(self, values, off=SO):
        """a source buffer holding `values` behind `off` random elements"""
        return self.up(np.concatenate([self.randn(off), np.asarray(values, f32).ravel()]))

    def dst(self, n, off=DO):
        return self.up(np.full(off + n + PAD, SENTINEL, f32))

    def prog(self, ops):
        return DeviceProgram(ops=ops, buffer_sizes=list(self.sizes), initial_uploads=list(self.ups))


def cdiv(a, b):
    return -(-a // b)


# ── the launcher rules, restated ──────────────────────────────────────────────────────────────────────────────────────────

def row_route(rows, cols, fused=False):
    """(form, split) of a stand-alone rmsnorm / a fused row chain over distinct buffers, switches at their defaults.
    kernels_generic.hip launch_rmsnorm :1284 (cols <= 32 * 256: the row chain kernel, else rmsnorm_kernel); launch_row_chain
    :1298-1300 (split doubles while it stays <= chunks, divides them, and rows * split * 2 <= 256), :1316 (no split in the looping
    form), :1317-1324 (NPT 4 / 16 / 32 up to 1024 / 4096 / 8192 columns, else the looping form)."""
    chunks, split = cdiv(cols, 256), 1
    while split * 2 <= chunks and rows * split * 2 <= 256 and chunks % (split * 2) == 0:
        split *= 2
    if cols <= 1024:
        return "npt4", split
    if cols <= 4096:
        return "npt16", split
    if cols <= 8192:
        return "npt32", split
    return ("loop" if fused else "rmsnorm_kernel"), 1


def dense_route(geom, a_off=None, b_off=None):
    """kernels_generic.hip launch_dense_matmul :1469 (b_cs == 1 and b_rs != 1: ncontig), :1475-1491 (b_rs == 1: K-contiguous; four-wide
    when a_cs == 1, K, a_rs and b_cs are multiples of 4 and both pointers are 16-byte aligned; of those M == 1 with K <= 1024
    streams), :1493 (else strided). f32 B only."""
    a_off = geom.a_offset if a_off is None else a_off
    b_off = geom.b_offset if b_off is None else b_off
    if geom.b_col_stride == 1 and geom.b_row_stride != 1:
        return "ncontig"
    if geom.b_row_stride == 1:
        vec = (geom.a_col_stride == 1 and geom.K % 4 == 0 and geom.a_row_stride % 4 == 0 and geom.b_col_stride % 4 == 0 and
               a_off % 4 == 0 and b_off % 4 == 0)
        if vec and geom.M == 1 and geom.K <= 1024:
            return "stream"
        return "kcontig4" if vec else "kcontig1"
    return "strided"


def chain_route(n, aligned, operand_is_earlier_store):
    """kernels_generic.hip launch_eltwise_chain :1258 (four per thread from 2^20 elements on, n % 4 == 0, every pointer 16-byte
    aligned), :1261-1262 (an operand an earlier step stored: step by step), :1264-1269."""
    if operand_is_earlier_store:
        return "step"
    return "pre4" if n >= 1 << 20 and n % 4 == 0 and aligned else "pre1"


# ── bounds ────────────────────────────────────────────────────────────────────────────────────────────────────────────────

def rows_D(cols, oracle=False):
    return cols // 8 + 8 if oracle else cdiv(cols, 256)


def layernorm_ref(x, D):
    """float64 layernorm of the rows of x and the bound of the module docstring for a summation depth D"""
    cols = x.shape[1]
    mu = x.mean(axis=1, keepdims=True)
    d = x - mu
    s2 = (d * d).sum(axis=1, keepdims=True)
    var = s2 / cols
    inv_std = 1.0 / np.sqrt(var + EPS)
    want = d * inv_std
    dmu = (D + 11) * U * np.abs(x).mean(axis=1, keepdims=True)
    cross = 2 * dmu * np.abs(d).sum(axis=1, keepdims=True) + cols * dmu * dmu
    rel_v = (D + 12) * U + np.divide(cross, s2, out=np.zeros_like(s2), where=s2 > 0)
    rel_i = 0.5 * rel_v * var / (var + EPS) + 3 * U
    return want, inv_std * (dmu + U * np.abs(d)) + np.abs(want) * (rel_i + U)


def softmax_ref(x):
    """float64 softmax with the reference's rules: the max ignores NaN, a non-finite shifted value counts 0, an empty sum gives 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax.reduce(np.concatenate([np.full((x.shape[0], 1), -np.inf), x], axis=1), axis=1, keepdims=True)
        sh = x - m
        e = np.where(np.isfinite(sh), np.exp(np.where(np.isfinite(sh), sh, 0.0)), 0.0)
        s = e.sum(axis=1, keepdims=True)
        return e * np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)


def softmax_bound(want, D):
    return (2e-6 + (D + 12) * U) * want + 1e-30


# ── rows: rmsnorm and the row chain ──────────────────────────────────────────────────────────────────────────────────────

ROW_SHAPES = (((1, 1), ("npt4", 1)), ((1, 255), ("npt4", 1)), ((1, 256), ("npt4", 1)), ((1, 257), ("npt4", 2)),
              ((2, 1000), ("npt4", 4)), ((3, 1024), ("npt4", 4)), ((3, 1025), ("npt16", 1)), ((2, 1536), ("npt16", 2)),
              ((5, 2560), ("npt16", 2)), ((2, 4096), ("npt16", 16)), ((2, 4097), ("npt32", 1)), ((2, 7936), ("npt32", 1)),
              ((2, 8192), ("npt32", 32)), ((2, 8193), None), ((128, 512), ("npt4", 2)), ((129, 1024), ("npt4", 1)))
NOSPLIT_COLS = (1000, 4096, 8192)
NOSPLIT_ROWS = 300


def _rms64(h):
    return h / np.sqrt((h * h).mean(axis=1, keepdims=True) + EPS)


def _rows_case(name, rows, cols, fused, want_route, x=None, y=None, g=None, oracle_rows=(), exact_rows=()):
    """stand-alone rmsnorm or add -> rmsnorm -> mul; rows in `oracle_rows` are compared with the oracle's bits instead of float64"""
    b = _B(name)
    n = rows * cols
    x = b.randn(n) if x is None else np.asarray(x, f32).ravel()
    D, Do = rows_D(cols), rows_D(cols, oracle=True)
    row_of = np.arange(n) // cols
    by_ref = ~np.isin(row_of, list(oracle_rows))
    idx = DO + np.arange(n)
    exact = np.isin(row_of, list(exact_rows))[by_ref] if len(exact_rows) else None

    def bounded(buf, want, extra, what):
        want = want.ravel()
        out = [Check(buf, idx[by_ref], want[by_ref], (D + extra) * U * np.abs(want[by_ref]), (Do + extra) * U * np.abs(want[by_ref]),
                     exact=exact, what=what)]
        if not by_ref.all():
            out.append(Check(buf, idx[~by_ref], mode="oracle", what=what + " (overflowing rows)"))
        return out

    if not fused:
        X, Dst = b.src(x), b.dst(n)
        ops = [DeviceOp.rmsnorm(Dst, X, rows, cols, EPS, src_offset=SO, dst_offset=DO)]
        checks = bounded(Dst, _rms64(x.astype(f64).reshape(rows, cols)), 16, "rmsnorm")
        launches = ()
    else:
        y = b.randn(n) if y is None else np.asarray(y, f32).ravel()
        g = b.randn(n) if g is None else np.asarray(g, f32).ravel()
        X, Y, G = b.src(x), b.src(y), b.src(g)
        H, NRM, O = b.dst(n), b.dst(n), b.dst(n)
        ops = [DeviceOp.elementwise("add", H, X, Y, n, dst_offset=DO, src0_offset=SO, src1_offset=SO),
               DeviceOp.rmsnorm(NRM, H, rows, cols, EPS, src_offset=DO, dst_offset=DO),
               DeviceOp.elementwise("mul", O, NRM, G, n, dst_offset=DO, src0_offset=DO, src1_offset=SO)]
        h64 = x.astype(f64) + y.astype(f64)
        nrm = _rms64(h64.reshape(rows, cols)).ravel()
        checks = [Check(H, idx, x + y, mode="bits", what="sum")] + bounded(NRM, nrm, 16, "norm") + bounded(O, nrm * g.astype(f64), 18, "product")
        launches = ((K_RMS, 3, 0, 2),)
    return Case(name, "rows", b.prog(ops), checks, launches, row_route(rows, cols, fused), want_route,
                info=dict(rows=rows, cols=cols, fused=fused, x=x, y=y, g=g))


def _row_specials(fused):
    cols = 1000
    b = _B("row_specials")
    x = np.stack([np.zeros(cols, f32), np.full(cols, 1e-20, f32), np.full(cols, 1e20, f32), b.randn(cols)])
    # (fused: + 0, so the rows stay what they are; the gain is random)
    return _rows_case(f"rows_specials_{'chain' if fused else 'rmsnorm'}", 4, cols, fused, ("npt4", 4), x=x, y=np.zeros(4 * cols, f32),
                      oracle_rows=(2,), exact_rows=(0,))


def nosplit_case(cols):
    """rows 0 and 1 of the fused (2, cols) case as rows 0 and 299 of a (300, cols) program with the same ops: rows * 2 > 256, so one
    workgroup per row. The case's checks name those two rows of the three stored buffers."""
    small = build_case(f"chain_2x{cols}")
    rows = NOSPLIT_ROWS
    b = _B(f"nosplit_{cols}")
    arrs = []
    for key in ("x", "y", "g"):
        a = b.randn(rows * cols).reshape(rows, cols)
        a[0], a[rows - 1] = small.info[key].reshape(2, cols)
        arrs.append(a)
    c = _rows_case(f"nosplit_{cols}", rows, cols, True, None, *arrs)
    sel = np.concatenate([np.arange(cols), (rows - 1) * cols + np.arange(cols)])
    c.info["pairs"] = [(big.buf, DO + sel, sm.buf, sm.idx) for big, sm in zip(c.checks, small.checks)]
    c.info["small"] = small
    return c


# ── softmax and layernorm ────────────────────────────────────────────────────────────────────────────────────────────────

SM_SHAPES = ((1, 1), (3, 7), (2, 255), (2, 256), (2, 257), (4, 1000))


def _rowwise_case(name, kind, rows, cols, x=None, exact01=False, exact_rows=()):
    """out of place into a sentinel buffer and in place over a copy of the source, same offsets"""
    b = _B(name)
    n = rows * cols
    x = b.randn(n) if x is None else np.asarray(x, f32).ravel()
    X, Dst, IP = b.src(x), b.dst(n), b.up(np.concatenate([b.randn(SO), x, b.randn(PAD)]))
    mk = DeviceOp.softmax if kind == "softmax" else DeviceOp.layernorm
    ops = [mk(Dst, X, rows, cols, src_offset=SO, dst_offset=DO), mk(IP, IP, rows, cols, src_offset=SO, dst_offset=SO)]
    x64 = x.astype(f64).reshape(rows, cols)
    D = cdiv(cols, 256)
    exact = None
    if kind == "softmax":
        want = softmax_ref(x64)
        bound, obound = softmax_bound(want, D), softmax_bound(want, cols)
        if exact01:
            exact = ((want == 0) | (want == 1)).ravel()
    else:
        want, bound = layernorm_ref(x64, D)
        obound = layernorm_ref(x64, cols)[1]
        if len(exact_rows):
            exact = np.isin(np.arange(n) // cols, list(exact_rows))
    idx = DO + np.arange(n)
    checks = [Check(Dst, idx, want.ravel(), bound.ravel(), obound.ravel(), exact=exact, what=kind),
              Check(IP, SO + np.arange(n), mode="same", same=(Dst, idx), what=kind + " in place")]
    return Case(name, kind, b.prog(ops), checks, info=dict(rows=rows, cols=cols))


def _softmax_specials():
    cols = 300
    b = _B("softmax_specials")
    r0 = np.full(cols, -np.inf, f32)
    r0[17] = 0.5
    r1 = np.full(cols, 1.25, f32)
    r2 = b.randn(cols)
    r2[::7] = 1e30
    r2[3::11] = -1e30
    r3 = b.randn(cols)
    r3[101] = np.inf
    r4 = b.randn(cols)
    r4[257] = np.nan
    return _rowwise_case("softmax_specials", "softmax", 5, cols, np.stack([r0, r1, r2, r3, r4]), exact01=True)


def _layernorm_specials():
    """row 0 is constant 2.0: every partial sum, in any order, is exact, so the mean is 2 and the row comes out as exact zeros"""
    cols = 300
    b = _B("layernorm_specials")
    x = np.stack([np.full(cols, 2.0, f32), (1e4 + b.rng.standard_normal(cols)).astype(f32)])
    return _rowwise_case("layernorm_specials", "layernorm", 2, cols, x, exact_rows=(0,))


# ── reduce ───────────────────────────────────────────────────────────────────────────────────────────────────────────────

REDUCE_SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (3, 1000), (4, 64), (5, 129), (9, 4097))


def _reduce_case(name, n_out, rs, x=None):
    """sum and max of the same rows into one destination, sum at DO, max one element behind the sums"""
    b = _B(name)
    x = b.randn(n_out * rs) if x is None else np.asarray(x, f32).ravel()
    X, Dst = b.src(x), b.dst(2 * n_out + 1)
    max_off = DO + n_out + 1
    ops = [DeviceOp.reduce("sum", Dst, X, n_out, rs, src_offset=SO, dst_offset=DO), DeviceOp.reduce("max", Dst, X, n_out, rs, src_offset=SO, dst_offset=max_off)]
    x2 = x.reshape(n_out, rs)
    with np.errstate(invalid="ignore"):
        s = x2.astype(f64).sum(axis=1)
        a = np.abs(x2.astype(f64)).sum(axis=1)
    a = np.where(np.isfinite(a), a, 0.0)
    mx = np.fmax.reduce(np.concatenate([np.full((n_out, 1), -np.inf, f32), x2], axis=1), axis=1)  # NaN-ignoring, -inf when empty
    checks = [Check(Dst, DO + np.arange(n_out), s, (cdiv(rs, 64) + 6) * U * a, (rs + 6) * U * a, what="sum"),
              Check(Dst, max_off + np.arange(n_out), mx.astype(f32), mode="bits", what="max")]
    return Case(name, "reduce", b.prog(ops), checks, info=dict(n_out=n_out, reduce_size=rs))


def _reduce_specials():
    rs = 130
    b = _B("reduce_specials")
    r0 = np.full(rs, -np.inf, f32)
    r1 = b.randn(rs)
    r1[[0, 64, 65, 129]] = np.nan
    r2 = b.randn(rs)
    r2[0::4], r2[2::4] = 1e8, -1e8
    return _reduce_case("reduce_specials", 3, rs, np.stack([r0, r1, r2]))


# ── dense f32 matmul ─────────────────────────────────────────────────────────────────────────────────────────────────────

def _G(M, K, N, a_rs, a_cs, b_rs, b_cs, a_off=SO, b_off=SO, dst_off=DO, dst_rs=None):
    return MatMulGeometry(M, N, K, a_rs, a_cs, b_rs, b_cs, a_off, b_off, dst_off, N if dst_rs is None else dst_rs)


DENSE = {  # name -> (geometry, route, c of the bound as a function of K)
    "dense_ncontig_1x1x1": (_G(1, 1, 1, 1, 1, 2, 1), "ncontig", lambda K: K),  # (b_rs = 2: with b_rs = 1 a single column counts as K-contiguous)
    "dense_ncontig_a_colmajor_dst_strided": (_G(3, 65, 257, 1, 3, 257, 1, dst_rs=260), "ncontig", lambda K: K),
    "dense_kcontig4": (_G(2, 260, 9, 260, 1, 1, 260, a_off=4, b_off=8), "kcontig4", lambda K: 4 * cdiv(K, 256) + 6),
    "dense_kcontig1_k_mod_4": (_G(3, 67, 5, 67, 1, 1, 67, a_off=0, b_off=0), "kcontig1", lambda K: cdiv(K, 64) + 6),
    "dense_kcontig1_a_cs": (_G(2, 64, 5, 4, 8, 1, 64, a_off=0, b_off=0), "kcontig1", lambda K: cdiv(K, 64) + 6),
    "dense_kcontig1_b_cs": (_G(2, 64, 5, 64, 1, 1, 65, a_off=0, b_off=0), "kcontig1", lambda K: cdiv(K, 64) + 6),
    "dense_kcontig1_a_offset": (_G(2, 64, 5, 64, 1, 1, 64, a_off=1, b_off=0), "kcontig1", lambda K: cdiv(K, 64) + 6),
    "dense_strided": (_G(2, 33, 300, 33, 1, 2, 66), "strided", lambda K: K),
}


def _dense_case(name):
    g, route, c = DENSE[name]
    b = _B(name)
    M, K, N = g.M, g.K, g.N
    ai = g.a_offset + np.arange(M)[:, None] * g.a_row_stride + np.arange(K)[None, :] * g.a_col_stride
    bi = g.b_offset + np.arange(K)[:, None] * g.b_row_stride + np.arange(N)[None, :] * g.b_col_stride
    di = g.dst_offset + np.arange(M)[:, None] * g.dst_row_stride + np.arange(N)[None, :]
    a, bm = b.randn(int(ai.max()) + 1), b.randn(int(bi.max()) + 1)
    A, Bm, Dst = b.up(a), b.up(bm), b.dst(int(di.max()) + 1, 0)
    A64, B64 = a[ai].astype(f64), bm[bi].astype(f64)
    mag = (np.abs(A64) @ np.abs(B64)).ravel()
    checks = [Check(Dst, di.ravel(), (A64 @ B64).ravel(), c(K) * U * mag, (K + 1) * U * mag, what="matmul")]
    return Case(name, "dense", b.prog([DeviceOp.matmul(Dst, A, Bm, g)]), checks, route=(dense_route(g),), want_route=(route,))


# ── elementwise ──────────────────────────────────────────────────────────────────────────────────────────────────────────

ELT_OPS = ("add", "mul", "neg", "abs", "sgn", "step", "relu", "sqrt", "recip", "exp", "log", "gelu")
ELT_NS = (1, 255, 256, 257, 1000)
EXACT_OPS = ("add", "mul", "neg", "abs", "sgn", "step", "sqrt", "recip")


def np_op(op, a, b=None):
    """(mode, want, bound): the op restated in numpy — float32 for the exactly rounded ops, float64 for exp / log / gelu"""
    with np.errstate(all="ignore"):
        if op in EXACT_OPS or op == "relu":
            one, zero = f32(1), f32(0)
            want = {"add": lambda: a + b, "mul": lambda: a * b, "neg": lambda: -a, "abs": lambda: np.abs(a),
                    "sgn": lambda: np.where(a > 0, one, np.where(a < 0, -one, zero)), "step": lambda: np.where(a > 0, one, zero),
                    "relu": lambda: np.fmax(a, zero), "sqrt": lambda: np.sqrt(a), "recip": lambda: one / a}[op]()
            return ("value" if op == "relu" else "bits"), want.astype(f32), None
        x = a.astype(f64)
        if op == "exp":
            want = np.exp(x)
        elif op == "log":
            want = np.log(x)
        else:
            want = 0.5 * x * (1.0 + np.tanh(0.7978845608 * (x + 0.044715 * x * x * x)))
        return "bound", want, 2e-6 * np.abs(np.where(np.isfinite(want), want, 0.0)) + 1e-6


def _elt_inputs(b, op, n):
    x = b.randn(n)
    if op in ("sqrt", "log"):
        x = np.abs(x) + f32(0.1)
    if op == "gelu":
        x = np.clip(x, -8, 8)
    return x.astype(f32), b.randn(n)


def _elt_case(op):
    """one program per op: n = 1, 255, 256, 257, 1000 out of the same sources, then the special values (for add / mul: every pair)"""
    b = _B("elt_" + op)
    x, y = _elt_inputs(b, op, max(ELT_NS))
    X, Y = b.src(x), b.src(y)
    ops, checks = [], []
    for n in ELT_NS:
        Dst = b.dst(n)
        ops.append(DeviceOp.elementwise(op, Dst, X, Y, n, dst_offset=DO, src0_offset=SO, src1_offset=SO))
        mode, want, bound = np_op(op, x[:n], y[:n])
        checks.append(Check(Dst, DO + np.arange(n), want, bound, bound, mode=mode, what=f"{op} n={n}"))
    sp = SPECIALS[(np.abs(SPECIALS) <= 8) | np.isnan(SPECIALS)] if op == "gelu" else SPECIALS
    xs, ys = (np.repeat(sp, sp.size), np.tile(sp, sp.size)) if op in ("add", "mul") else (sp, sp[::-1].copy())
    XS, YS, Dst = b.src(xs), b.src(ys), b.dst(xs.size)
    ops.append(DeviceOp.elementwise(op, Dst, XS, YS, xs.size, dst_offset=DO, src0_offset=SO, src1_offset=SO))
    mode, want, bound = np_op(op, xs, ys)
    checks.append(Check(Dst, DO + np.arange(xs.size), want, bound, bound, mode=mode, what=f"{op} special values"))
    return Case("elt_" + op, "eltwise", b.prog(ops), checks, info=dict(op=op))


# ── elementwise chains ───────────────────────────────────────────────────────────────────────────────────────────────────

def _chain_add_mul(name, n, so, do, want_route):
    """t = x + y; z = t * w"""
    b = _B(name)
    x, y, w = b.randn(n), b.randn(n), b.randn(n)
    X, Y, W, T, Z = b.src(x, so), b.src(y, so), b.src(w, so), b.dst(n, do), b.dst(n, do)
    ops = [DeviceOp.elementwise("add", T, X, Y, n, dst_offset=do, src0_offset=so, src1_offset=so),
           DeviceOp.elementwise("mul", Z, T, W, n, dst_offset=do, src0_offset=do, src1_offset=so)]
    t = x + y
    idx = do + np.arange(n)
    checks = [Check(T, idx, t, mode="bits", what="t = x + y"), Check(Z, idx, t * w, mode="bits", what="z = t * w")]
    aligned = so % 4 == 0 and do % 4 == 0
    return Case(name, "chains", b.prog(ops), checks, ((K_FUSED, 2, 0, 1),), (chain_route(n, aligned, False),), (want_route,))


def _chain_fallback():
    """t = x + y; u = -t; z = u * t: the last step's operand is step 0's store at the same index"""
    n = 1000
    b = _B("chain_operand_is_earlier_store")
    x, y = b.randn(n), b.randn(n)
    X, Y, T, Un, Z = b.src(x), b.src(y), b.dst(n), b.dst(n), b.dst(n)
    ops = [DeviceOp.elementwise("add", T, X, Y, n, dst_offset=DO, src0_offset=SO, src1_offset=SO),
           DeviceOp.elementwise("neg", Un, T, T, n, dst_offset=DO, src0_offset=DO, src1_offset=DO),
           DeviceOp.elementwise("mul", Z, Un, T, n, dst_offset=DO, src0_offset=DO, src1_offset=DO)]
    t = x + y
    idx = DO + np.arange(n)
    checks = [Check(T, idx, t, mode="bits", what="t"), Check(Un, idx, -t, mode="bits", what="u = -t"), Check(Z, idx, -t * t, mode="bits", what="z = u * t")]
    return Case("chain_operand_is_earlier_store", "chains", b.prog(ops), checks, ((K_FUSED, 3, 0, 2),), (chain_route(n, False, True),), ("step",))


def _chain_silu():
    """the SiLU pair of fused ops of test_elementwise_all_ops_and_fused_chain: [neg, exp]; [add 1, recip, mul x (swapped)].
    e = exp(-x) under the elementwise bar; x / (1 + e): the bar's 2e-6 (times e / (1 + e) < 1) and three more roundings."""
    n = 257
    b = _B("chain_silu")
    x = b.randn(n)
    X, One, E, S = b.src(x), b.src(np.ones(n, f32)), b.dst(n), b.dst(n)
    ops = [DeviceOp.fused_elementwise([FusedEwStep("neg"), FusedEwStep("exp")], n, E, X, dst_offset=DO, src_offset=SO),
           DeviceOp.fused_elementwise([FusedEwStep("add", False, One, SO), FusedEwStep("recip"), FusedEwStep("mul", True, X, SO)], n, S, E,
                                      dst_offset=DO, src_offset=DO)]
    e = np.exp(-x.astype(f64))
    s = x.astype(f64) / (1 + e)
    idx = DO + np.arange(n)
    be, bs = 2e-6 * e + 1e-6, (2e-6 + 3 * U) * np.abs(s) + 1e-6
    checks = [Check(E, idx, e, be, be, what="exp(-x)"), Check(S, idx, s, bs, bs, what="silu")]
    return Case("chain_silu", "chains", b.prog(ops), checks, ((K_FUSED, 2, 0, 1),), (chain_route(n, False, False),), ("pre1",))


CHAIN13 = ("add", "mul", "neg", "abs", "sqrt", "add", "mul_swapped", "abs", "recip", "neg", "add", "mul", "abs")


def _chain_13():
    """thirteen exactly rounded ops, each consuming its predecessor: kMaxChainSteps = 12 (kernels.h) cuts the chain behind op 11"""
    n = 1000
    b = _B("chain_13_ops")
    x, y, w = b.randn(n), b.randn(n), b.randn(n)
    X, Y, W = b.src(x), b.src(y), b.src(w)
    ops, checks = [], []
    cur, cur_off, v = X, SO, x
    for name in CHAIN13:
        Dst = b.dst(n)
        if name == "mul_swapped":
            ops.append(DeviceOp.elementwise("mul", Dst, W, cur, n, dst_offset=DO, src0_offset=SO, src1_offset=cur_off))
            v = np_op("mul", w, v)[1]
        else:
            other = Y if name == "add" else W
            ops.append(DeviceOp.elementwise(name, Dst, cur, other, n, dst_offset=DO, src0_offset=cur_off, src1_offset=SO))
            v = np_op(name, v, y if name == "add" else w)[1]
        checks.append(Check(Dst, DO + np.arange(n), v, mode="bits", what=f"step {len(ops) - 1} {name}"))
        cur, cur_off = Dst, DO
    assert len(ops) == 13
    return Case("chain_13_ops", "chains", b.prog(ops), checks, ((K_FUSED, 12, 0, 11), (K_ELT, 1, 12, 12)), (chain_route(n, False, False),), ("pre1",))


# ── repeat: one level, four ops of four sizes ────────────────────────────────────────────────────────────────────────────

def _repeat_case():
    b = _B("repeat_level")
    S1, S2, S3, S4 = b.up(b.randn(SO + 1)), b.up(b.randn(SO + 2)), b.up(b.randn(SO + 7)), b.up(b.randn(16))
    D1, D2, D3, D4 = b.dst(1000), b.dst(1), b.dst(259), b.dst(24)
    ops = [DeviceOp.repeat(D1, S1, 1000, (1, 1, 1, 1), (1000, 1, 1, 1), (1, 1, 1, 1), (1, 1000, 1000, 1000), src_offset=SO, dst_offset=DO),  # mode 1
           DeviceOp.repeat(D2, S2, 1, (2, 1, 1, 1), (1, 1, 1, 1), (1, 2, 2, 2), (1, 1, 1, 1), src_offset=SO, dst_offset=DO),                 # mode 2
           DeviceOp.repeat(D3, S3, 259, (7, 1, 1, 1), (259, 1, 1, 1), (1, 7, 7, 7), (1, 259, 259, 259), src_offset=SO, dst_offset=DO),      # mode 3
           DeviceOp.repeat(D4, S4, 24, (3, 2, 1, 1), (6, 4, 1, 1), (1, 4, 8, 8), (1, 6, 24, 24), src_offset=1, dst_offset=DO)]              # generic
    checks = [Check(d, DO + np.arange(n), mode="oracle", what=f"repeat {i}") for i, (d, n) in enumerate(((D1, 1000), (D2, 1), (D3, 259), (D4, 24)))]
    c = Case("repeat_level", "repeat", b.prog(ops), checks, launches_after=((K_REPEAT, 4, 0, 3),))
    c.inputs = (ProgramIO(S3, c.upload(S3).copy()),)  # the same values, now written by the host: the repeats run in the plan
    return c


# ── movement: a rope and two slice_assigns of three sizes in one launch ──────────────────────────────────────────────────

MOVE_POSITIONS = (0, 3, 7)


def _move_case():
    b = _B("move_level")
    hd, seq, kv_dim = 32, 5, 192
    XR, CS, DR = b.up(b.randn(kv_dim * seq)), b.up(b.randn(4 * hd * seq)), b.dst(2 * hd * seq)
    rope = DeviceOp.rope(DR, XR, CS, hd, seq, src_off=64, cs_off=0, dst_off=DO, src_rs=1, src_cs=kv_dim, cs_cs=4 * hd)
    SA, DA = b.src(b.randn(3 * 8)), b.dst(6 * 2 + 2 * 15 + 1)
    small = DeviceOp.slice_assign(DA, SA, 7, 3, dst_base_offset=0, dst_offset=DO, dst_row_stride=2, dst_col_stride=15, src_offset=SO, src_row_stride=1,
                                  src_col_stride=8, patch_stride=0)
    rows, width = 300, 8  # a [3][300][8] cache: column `pos` of every row, one position per execute
    SB, DB = b.src(b.randn(3 * rows)), b.dst(3 * rows * width)
    dyn = DeviceOp.slice_assign(DB, SB, rows, 3, dst_base_offset=DO, dst_offset=DO + MOVE_POSITIONS[0], dst_row_stride=width, dst_col_stride=rows * width,
                                src_offset=SO, src_row_stride=1, src_col_stride=rows, patch_stride=1)
    everything = lambda buf: np.arange(b.sizes[buf])  # noqa: E731
    checks = [Check(buf, everything(buf), mode="oracle", what=what) for buf, what in ((DR, "rope"), (DA, "slice_assign 7x3"), (DB, "slice_assign 300x3"))]
    refresh = tuple([rope, small, dyn.with_(dst_offset=DO + pos)] for pos in MOVE_POSITIONS[1:])
    return Case("move_level", "move", b.prog([rope, small, dyn]), checks, ((K_MOVE, 3, 0, 2),), refresh=refresh)


# ── the table ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def _table():
    """name -> (group, builder)"""
    t = {}
    for (rows, cols), route in ROW_SHAPES:
        t[f"rmsnorm_{rows}x{cols}"] = "rows", lambda r=rows, c=cols, w=route: _rows_case(f"rmsnorm_{r}x{c}", r, c, False, w or ("rmsnorm_kernel", 1))
        t[f"chain_{rows}x{cols}"] = "rows", lambda r=rows, c=cols, w=route: _rows_case(f"chain_{r}x{c}", r, c, True, w or ("loop", 1))
    t["rows_specials_rmsnorm"] = "rows", lambda: _row_specials(False)
    t["rows_specials_chain"] = "rows", lambda: _row_specials(True)
    for kind in ("softmax", "layernorm"):
        for rows, cols in SM_SHAPES:
            t[f"{kind}_{rows}x{cols}"] = kind, lambda k=kind, r=rows, c=cols: _rowwise_case(f"{k}_{r}x{c}", k, r, c)
    t["softmax_specials"] = "softmax", _softmax_specials
    t["layernorm_specials"] = "layernorm", _layernorm_specials
    for n_out, rs in REDUCE_SHAPES:
        t[f"reduce_{n_out}x{rs}"] = "reduce", lambda o=n_out, r=rs: _reduce_case(f"reduce_{o}x{r}", o, r)
    t["reduce_specials"] = "reduce", _reduce_specials
    for name in DENSE:
        t[name] = "dense", lambda n=name: _dense_case(n)
    for op in ELT_OPS:
        t["elt_" + op] = "eltwise", lambda o=op: _elt_case(o)
    for n in (1, 257, 1000):
        t[f"chain_add_mul_{n}"] = "chains", lambda n=n: _chain_add_mul(f"chain_add_mul_{n}", n, SO, DO, "pre1")
    t["chain_add_mul_vec4"] = "chains", lambda: _chain_add_mul("chain_add_mul_vec4", 1 << 20, 0, 0, "pre4")
    t["chain_add_mul_unaligned"] = "chains", lambda: _chain_add_mul("chain_add_mul_unaligned", (1 << 20) + 4, 1, 0, "pre1")
    t["chain_operand_is_earlier_store"] = "chains", _chain_fallback
    t["chain_silu"] = "chains", _chain_silu
    t["chain_13_ops"] = "chains", _chain_13
    t["repeat_level"] = "repeat", _repeat_case
    t["move_level"] = "move", _move_case
    return t


_TABLE = _table()
CASE_NAMES = tuple(_TABLE)
GROUPS = ("rows", "softmax", "layernorm", "reduce", "dense", "eltwise", "chains", "repeat", "move")


def build_case(name):
    group, make = _TABLE[name]
    c = make()
    assert (c.name, c.group) == (name, group)
    return c


def names_of(group):
    return tuple(n for n, (g, _) in _TABLE.items() if g == group)


# ── comparing ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def same_bits(a, b):
    """equal bits, or NaN on both sides"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(b)
    return a.shape == b.shape and bool(np.isnan(a[nan]).all()) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def hold(check, bufs, which="bound", oracle_bufs=None):
    """assert one Check on `bufs` (buffer -> flat f32 array); returns the largest error / bound of a "bound" check, else 0"""
    got = bufs[check.buf][check.idx]
    what = check.what
    if check.mode == "bound":
        want, bound = check.want, getattr(check, which)
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin].astype(f64), want[~fin], equal_nan=True), f"{what}: non-finite values differ"
        assert np.isfinite(got[fin]).all(), f"{what}: {np.count_nonzero(~np.isfinite(got[fin]))} non-finite values"
        err = np.abs(got[fin].astype(f64) - want[fin])
        ratio = np.divide(err, bound[fin], out=np.where(err > 0, np.inf, 0.0), where=bound[fin] > 0)
        worst = float(ratio.max()) if ratio.size else 0.0
        assert worst <= 1.0, f"{what}: error / bound = {worst:.3g} at {int(np.argmax(ratio))} (|error| {float(err.max()):.3g})"
        if check.exact is not None:
            assert np.array_equal(got[check.exact].astype(f64), want[check.exact]), f"{what}: not exact where it has to be"
        return worst
    if check.mode == "bits":
        assert same_bits(got, check.want), f"{what}: bits differ from numpy float32 at {np.flatnonzero(~_eq(got, check.want))[:8]}"
    elif check.mode == "value":
        nan = np.isnan(check.want)
        assert np.isnan(got[nan]).all() and np.array_equal(got[~nan], check.want[~nan]), f"{what}: values differ"
    elif check.mode == "oracle":
        assert same_bits(got, oracle_bufs[check.buf][check.idx]), f"{what}: bits differ from the oracle"
    elif check.mode == "same":
        assert same_bits(got, bufs[check.same[0]][check.same[1]]), f"{what}: bits differ from the out-of-place result"
    return 0.0


def _eq(a, b):
    return (a.view(np.uint32) == np.asarray(b, f32).view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def untouched(case, bufs):
    """every checked buffer keeps its upload, bit for bit, outside what its checks name"""
    for buf in case.checked_buffers():
        keep = np.ones(case.prog.buffer_sizes[buf], bool)
        for c in case.checks:
            if c.buf == buf:
                keep[c.idx] = False
        up = case.upload(buf)
        assert np.array_equal(bufs[buf][keep].view(np.uint32), up[keep].view(np.uint32)), f"{case.name}: buffer {buf} written outside its span"


def ulps(check, bufs, floor=FLT_MIN):
    """largest |got - want| in units of the float32 spacing at want, over the finite |want| >= floor of a "bound" check (below the
    bar's atol an error in ulps says little: gelu near -8 cancels down to 1e-14)"""
    got, want = bufs[check.buf][check.idx].astype(f64), check.want
    fin = np.isfinite(want) & (np.abs(want) >= floor)
    return float((np.abs(got[fin] - want[fin]) / np.spacing(np.abs(want[fin]).astype(f32)).astype(f64)).max()) if fin.any() else 0.0


def run_oracle(be, case):
    """the case on an OracleBackend: every buffer after the first execute, after each refresh, and after the execute with inputs"""
    h = be.compileProgram(case.prog)
    assert h
    try:
        snap = lambda: [be.buffer(h, i).copy() for i in range(len(case.prog.buffer_sizes))]  # noqa: E731
        be.executeProgram(h, [], [])
        out = [snap()]
        for ops in case.refresh:
            be.refreshProgram(h, ops)
            be.executeProgram(h, [], [])
            out.append(snap())
        if case.inputs:
            be.executeProgram(h, list(case.inputs), [])
            out.append(snap())
        return out
    finally:
        be.freeProgram(h)
