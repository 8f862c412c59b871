"""Case table for the f16-promoted dense matmul (zgml_amd/csrc/dense_f16.hip; promotion in runtime.hip compile_program, grouping
in plan.hip make_single). No GPU and no HIP library here: the launchers' rules restated in Python, programs, float64 references.
tests/test_dense_f16_cases_host.py pins the table on the CPU, tests/test_hip_dense_f16_routes.py runs it on the device.

Restated rules (each cites what it restates):
  promoted(prog)   runtime.hip:776-808   which buffers keep only an MFMA-packed f16 image
  stream_nt(prog)  runtime.hip:885       the packed images together are >= 192 MiB: the launches load weights non-temporally
  route(...)       dense_f16.hip launch_dense_f16, launch_dense_f16_tile2, f16_tiles_per_wg: instantiation, waves, chunks per
                   loop trip, m-tiles, grid, column groups per workgroup
  plan(prog)       plan.hip:163-199 and dense_f16.hip dense_f16_can_group: which matmuls share a launch, which skip the A pack

Reference and bar (as tests/test_hip_dense_f16.py and tests/handover_cases.py): B rounded to f16, A rounded to
f16 for M > 1 only (np.float16 rounds to nearest even like __floats2half2_rn), products and sums in float64;
|got - want| <= 2e-5 * (|a'| @ |b'|) + 1e-30 per output over the rounded operands. A matmul whose promotion is refused is held to
the same bar over the unrounded operands.

f16 subnormal operands (measured by the f16_edges cases): the M = 1 kernel (v_fma_mix_f32) takes them at their value and stays on
the contract alone. The matrix instruction of the M > 1 kernels (v_mfma_f32_16x16x32_f16) does not flush them: every M > 1
f16_edges case but those at K = 64, N = 24576 meets the contract alone by 100x or more, the subnormal-only columns and the
subnormal A rows included, and check_mat holds them to it. At K = 64, N = 24576 about twenty of 393216 outputs are off by 2 to 5
units of 2^-24 where the contract allows 1.3 to 3.5 (1.47 to 2.38 of the bar, on the staged and on the tile kernel alike;
profiles/r25_dense_f16_parity.txt). Each of them has a 32-k dot that holds 0x0001 * 65504 (65504 units) next to products with a
subnormal operand 2^15 or more times smaller; the dots without such a mix are exact. Whether the small products are lost or
the large one is carried short is not settled (the figures fit both). That is the matrix cores', not the kernel's. An output of
an M > 1 form on f16_edges that misses the contract is therefore held to the contract plus subnormal_slack: the issue's term,
2^-14 * |other operand| per subnormal operand, counted only in the dots that mix magnitudes so (zero elsewhere). The
subnormal-only columns get no term, and at most MAX_SLACK_OUTPUTS outputs of a matmul may need one: a flushed operand in the
pack kernel or the instruction moves hundreds of outputs, those columns first, and fails. Every other profile, and the oracle
on every profile, stays on the contract alone.

Layout of every case: A rows with a_rs > K, NaN in the gaps, in front of a_offset and behind the last row; B with NaN in front of
b_offset and behind its last element (and in the gaps where b_rs > N or the K-contiguous form leaves any); dst with
dst_rs > N and the sentinel -7 in every word the matmul does not write.

Value profiles: `normal` (A ~ N(0, 1), B ~ 0.05 N(0, 1)); `f16_edges` (edges_b / edges_a below); `zero_row` (an all-zero A row
for M > 1 and an all-zero B column: exact zeros); `overflow` (weights of 70000 and -65520 in the last k of two columns, for
M > 1 also one a of -70000: the non-finite outputs and the sign of every inf must equal float64's over the rounded operands).
0x7BFF (65504) needs no scaling: with |a| of O(1) (or f16 edge values) and K <= 2080 every f32 sum stays below 2^44.

Shapes that differ from the issue's list: M = 16 at N = 20480 is added, without and with the filler, because
dense_f16_tile2_kernel<1, *, 2> is reached by nothing else; the overflow cases sit at K = 288, 800, 544, 1056 / 1030 / 2080
(KC is no multiple of the step at any of them).

Not covered: the NT instantiations of the env-only kernels (dense_f16_kernel<1 | 2, *, *, true>, the CG = 4 tile kernels with
NT, the narrow R = 2 forms with NT)."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, MatMulGeometry, ProgramIO, QuantizedWeightUpload

f32, f64, f16 = np.float32, np.float64, np.float16
TOL = 2e-5
FLOOR = 1e-30
SENTINEL = -7.0
NT_BYTES = 192 << 20    # runtime.hip:885
MAX_PARTS = 3           # dense_f16.hip kMaxF16Parts
FILLER_K, FILLER_N = 4096, 24576

DEFAULT_ENV = {"ZGML_F16_TILE2": 1, "ZGML_F16_TILE2_WIDE": 1, "ZGML_F16_TILE2_WAVES": 8, "ZGML_F16_TILE2_CG": 0, "ZGML_F16_GROUPS": 0}
# the switches only a process of its own can latch (switches.h:110-114), and the table each child runs
FORCED = {"staged": {"ZGML_F16_TILE2": 0}, "cg4": {"ZGML_F16_TILE2_CG": 4}, "narrow3": {"ZGML_F16_TILE2_WIDE": 0, "ZGML_F16_TILE2_WAVES": 3}}


def cdiv(a, b):
    return (a + b - 1) // b


def env_of(forced=None):
    return {**DEFAULT_ENV, **(forced or {})}


# ── restated rules ─────────────────────────────────────────────────────────────────────────────────────────────────────

def packed_bytes(K, N):
    """dense_f16.hip f16_packed_bytes"""
    return (N // 16) * cdiv(K, 32) * 64 * 16


def promoted(prog):
    """runtime.hip:776-808: {buffer: (K, N, b_offset, b_rs, b_cs)} of the buffers kept only as packed f16. B has an initial
    upload; every op that touches the buffer is a matmul using it as B with one geometry (so no op writes it, and it is no
    matmul's A or dst); a_col_stride == 1; N % 16 == 0 (f16_packable); a != b; dst != b."""
    has_upload = {io.buf_idx for io in prog.initial_uploads}
    state, geo = {}, {}
    for op in prog.ops:
        if op.kind != "matmul":
            for b in op.buffers():
                state[b] = -1
            continue
        g = op.geom
        state[op.dst] = -1  # (the schedule's writes of the op, :789)
        key = (g.K, g.N, g.b_offset, g.b_row_stride, g.b_col_stride)
        if op.a == op.b or op.dst == op.b or op.b not in has_upload or g.a_col_stride != 1 or not (g.K > 0 and g.N > 0 and g.N % 16 == 0):
            state[op.b] = -1
        elif state.get(op.b, 0) == 0:
            state[op.b], geo[op.b] = 1, key
        elif state[op.b] == 1 and geo[op.b] != key:
            state[op.b] = -1
        state[op.a] = -1
    return {b: geo[b] for b, s in state.items() if s == 1}


def stream_nt(prog):
    """runtime.hip:885"""
    return sum(packed_bytes(K, N) for K, N, *_ in promoted(prog).values()) >= NT_BYTES


def tiles_per_wg(M, env=None):
    """dense_f16.hip f16_tiles_per_wg"""
    wide = env_of(env)["ZGML_F16_TILE2_WIDE"]
    return 8 if M > 64 and wide else 4 if M > 32 and wide else 2 if M > 16 else 1


@dataclass(frozen=True)
class Route:
    name: str        # the instantiation
    tile2: bool
    R: int
    waves: int
    step: int        # 32-k chunks per loop trip (tile2: DEPTH * waves) or per step (dense_f16_kernel: depth * waves)
    tiles: int       # m-tiles the A operand is laid out for (tile2), or the 16-row tiles of the rows (staged)
    grid: tuple
    CG: int          # column groups per workgroup (staged form: G)
    lds: int

    def trips(self, K):
        return cdiv(cdiv(K, 32), self.step)

    def live_last(self, K):
        """chunks of the last trip that lie inside K; the others are clamped duplicates"""
        return cdiv(K, 32) - (self.trips(K) - 1) * self.step


def _b(v):
    return "true" if v else "false"


def route(M, K, Ns, a_aligned, a_rs, nt, env=None):
    """The launch of one matmul, or of a group over the same rows (Ns: the N of every part), with promoted weights.
    launch_dense_f16 (dense_f16.hip:467-510), launch_dense_f16_tile2 (:398-448)."""
    e = env_of(env)
    Ns = [Ns] if isinstance(Ns, int) else list(Ns)
    KC = cdiv(K, 32)
    if M > 1 and e["ZGML_F16_TILE2"]:  # dense_f16_scratch_bytes != 0: the pre-laid-out-A tile kernel
        R = tiles_per_wg(M, e)
        tiles = cdiv(cdiv(M, 16), R) * R
        waves = max(1, min(KC, e["ZGML_F16_TILE2_WAVES"]))
        groups = [n // 16 for n in Ns]
        CG = 1
        if R <= 2:
            if sum(groups) // 2 >= 640 and all(g % 2 == 0 for g in groups):
                CG = 2
            if e["ZGML_F16_TILE2_CG"] in (1, 2, 4) and all(g % e["ZGML_F16_TILE2_CG"] == 0 for g in groups):
                CG = e["ZGML_F16_TILE2_CG"]
        depth = 2 if R >= 8 else 3 if R >= 4 else 3 if CG >= 4 else 4
        nt_eff = bool(nt) and tiles // R == 1
        return Route(f"dense_f16_tile2_kernel<{R}, {_b(nt_eff)}, {CG}>", True, R, waves, depth * waves, tiles,
                     (sum(g // CG for g in groups), tiles // R), CG, waves * R * CG * 256 * 4)
    assert len(Ns) == 1
    NB2 = Ns[0] // 16
    R = 0 if M == 1 else 2 if M > 16 else 1
    depth, max_kw = (4, 8 if NB2 <= 384 else 4) if R == 2 else (8, 4)
    waves = min(cdiv(KC, depth), max_kw)
    xvec = bool(a_aligned) and K % 4 == 0 and (M == 1 or a_rs % 4 == 0)
    chf = waves * depth * 32
    if R == 0:
        return Route(f"dense_f16_kernel<0, {_b(xvec)}, 1, {_b(nt)}>", False, 0, waves, waves * depth, 1, (NB2, 1), 1, 2 * chf * 4)
    G = e["ZGML_F16_GROUPS"] or (2 if NB2 >= 1536 else 1)
    if waves * G > 8:
        G = 1
    lds = max(2 * 16 * R * ((chf + 8) // 2) * 4, waves * G * R * 256 * 4)
    return Route(f"dense_f16_kernel<{R}, {_b(xvec)}, {G}, {_b(nt)}>", False, R, waves, waves * depth, cdiv(M, 16),
                 (cdiv(NB2, G), cdiv(M, 16 * R)), G, lds)


def a_unpadded(M, K, env=None):
    """dense_f16.hip dense_f16_a_unpadded"""
    e = env_of(env)
    return M > 1 and M % 16 == 0 and K % 32 == 0 and (M // 16) % tiles_per_wg(M, e) == 0 and bool(e["ZGML_F16_TILE2"])


# The launch planner over programs of matmul / qmatmul ops alone (no producer in front of a matmul, so no hook arms one).
@dataclass
class PlannedLaunch:
    lo: int
    hi: int
    kind: str            # "f16" (promoted matmul), "dense" (f32 matmul), "q" (qmatmul), "other"
    reuse_a: bool = False
    parts: list = field(default_factory=list)   # op indices of an f16 launch


def _span(off, M, rs, n):
    return off, off + (M - 1) * rs + n


def _apart(x, y):
    """spans as (buffer, lo, hi): dense_f16_can_group compares device pointers; buffers never overlap each other"""
    return x[0] != y[0] or x[2] <= y[1] or y[2] <= x[1]


def can_group(p, q, env=None):
    """dense_f16.hip dense_f16_can_group over two promoted matmul ops of a program (stream_nt is one per program)"""
    g, h = p.geom, q.geom
    da, db = (p.dst, *_span(g.dst_offset, g.M, g.dst_row_stride, g.N)), (q.dst, *_span(h.dst_offset, h.M, h.dst_row_stride, h.N))
    rows = (p.a, *_span(g.a_offset, g.M, g.a_row_stride, g.K))
    return (g.M > 1 and bool(env_of(env)["ZGML_F16_TILE2"]) and (p.a, g.a_offset) == (q.a, h.a_offset) and g.M == h.M and g.K == h.K and
            g.a_row_stride == h.a_row_stride and _apart(da, db) and _apart(da, rows) and _apart(db, rows))


def q_splits(M, K, N):
    """the Q4_0 qmatmuls of this table (f16-exact scales, M = 32, K % 128 == 0) split their A rows into the shared scratch
    (qmatmul_scratch_bytes != 0; tests/handover_cases.py q4_arms)"""
    return M > 1 and K % 128 == 0


def plan(prog, env=None):
    """plan.hip:163-199 (reuse_a, joins) and :220-247 (the quantized split owns the scratch): the launches of a program of matmul
    and qmatmul ops. split state = (plan position, a buffer, a offset, M, K, a_rs, kind)."""
    e = env_of(env)
    weights = promoted(prog)
    out, split, group = [], None, None
    for i, op in enumerate(prog.ops):
        pos = len(out)
        if op.kind == "qmatmul":
            rs = op.input_row_stride or op.K
            if q_splits(op.M, op.K, op.N):
                split = (pos, op.input, op.input_offset, op.M, op.K, rs, 1)
            out.append(PlannedLaunch(i, i, "q"))
            group = None
            continue
        if op.kind != "matmul" or op.b not in weights:
            out.append(PlannedLaunch(i, i, "dense" if op.kind == "matmul" else "other"))
            continue
        g = op.geom
        if not (g.M > 1 and e["ZGML_F16_TILE2"]):  # no scratch for it: launch_dense_f16 directly, the split state is not touched
            out.append(PlannedLaunch(i, i, "f16", parts=[i]))
            continue
        key = (op.a, g.a_offset, g.M, g.K, g.a_row_stride, 2)
        reuse = split is not None and split[0] + 1 == pos and split[1:] == key
        split = (pos, *key)
        joins = reuse and group is not None and len(group.parts) < MAX_PARTS and all(can_group(prog.ops[t], op, e) for t in group.parts)
        if joins:
            group.parts.append(i)
            group.hi = i
            split = (pos - 1, *key)
            continue
        group = PlannedLaunch(i, i, "f16", reuse, [i])
        out.append(group)
    return out


def joins(prog, env=None):
    """[(op_lo, op_hi)] of the launches, as the plan text's `ops n [lo..hi]` gives them"""
    return [(L.lo, L.hi) for L in plan(prog, env)]


def reuse_a(prog, env=None):
    """{first op of an f16 tile launch: it skips pack_a_f16_kernel}"""
    return {L.lo: L.reuse_a for L in plan(prog, env) if L.kind == "f16" and prog.ops[L.lo].geom.M > 1 and env_of(env)["ZGML_F16_TILE2"]}


# ── value profiles ─────────────────────────────────────────────────────────────────────────────────────────────────────

CROSS = np.array([2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 2.0 ** -14 * (1 - 2.0 ** -12)], f32)  # -> 0 (tie to even), 0x0001, 0x0400
BELOW_INF = np.nextafter(f32(65520.0), f32(0))  # 65519.992: the largest f32 that still rounds to 0x7BFF


def _bits(rng, pats, shape):
    sign = rng.choice(np.array([0, 0x8000], np.uint16), shape)
    return (rng.choice(np.array(pats, np.uint16), shape) | sign).view(f16).astype(f32)


def _cross(rng, shape):
    return (rng.choice(CROSS, shape) * rng.choice(np.array([-1, 1], f32), shape)).astype(f32)


def edges_b(rng, K, N):
    """column n by n % 8: 0 subnormals and zeros only; 1 f32 values that round across a boundary (to 0, 0x0001, 0x0400);
    2 subnormals and the smallest normal; 3 every pattern, 0x3C00 and 0x7BFF among them; 4 a column of +-65519.992 alone;
    5 ones and zeros; 6 the largest subnormal only; 7 as `normal`. Both signs everywhere."""
    B = (rng.standard_normal((K, N)) * 0.05).astype(f32)
    cls = np.arange(N) % 8
    cols = [_bits(rng, [0x0001, 0x03FF, 0x0000], (K, N)), _cross(rng, (K, N)), _bits(rng, [0x0001, 0x03FF, 0x0400], (K, N)),
            _bits(rng, [0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x0000], (K, N)),
            (BELOW_INF * rng.choice(np.array([-1, 1], f32), (K, N))).astype(f32), _bits(rng, [0x3C00, 0x0000], (K, N)),
            _bits(rng, [0x03FF], (K, N))]
    for c, v in enumerate(cols):
        B[:, cls == c] = v[:, cls == c]
    return B


def edges_a(rng, M, K):
    """M > 1: row m by m % 4: 1 f16 subnormals, the smallest normal and zeros; 3 f32 values that round across a boundary"""
    A = rng.standard_normal((M, K)).astype(f32)
    if M > 1:
        row = np.arange(M) % 4
        A[row == 1] = _bits(rng, [0x0001, 0x03FF, 0x0400, 0x0000], (M, K))[row == 1]
        A[row == 3] = _cross(rng, (M, K))[row == 3]
    return A


def subnormal_only_columns(N):
    """f16_edges: the columns whose rounded weights are all f16 subnormals or zeros"""
    return [n for n in range(N) if n % 8 in (0, 6)]


def make_values(profile, rng, M, K, N):
    if profile == "f16_edges":
        return edges_a(rng, M, K), edges_b(rng, K, N)
    A = rng.standard_normal((M, K)).astype(f32)
    B = (rng.standard_normal((K, N)) * 0.05).astype(f32)
    if profile == "zero_row":
        if M > 1:
            A[min(5, M - 1)] = 0
        B[:, 3] = 0
    elif profile == "overflow":
        A[:, K - 1] = 1.5 * np.where(np.arange(M) % 2, -1, 1)
        B[K - 1, 5], B[K - 1, 9] = 70000.0, -65520.0  # both round to inf: 65520 is the tie, and ties go to even
        if M > 1:
            A[M // 2, 0] = -70000.0
    else:
        assert profile == "normal", profile
    return A, B


# ── cases ──────────────────────────────────────────────────────────────────────────────────────────────────────────────

@dataclass
class Mat:
    """one checked matmul: its op, where its operands lie, and the f32 values it reads"""
    op: int
    M: int
    K: int
    N: int
    a_buf: int
    a_off: int
    a_rs: int
    a_cs: int
    b_buf: int
    d_buf: int
    d_off: int
    d_rs: int
    A: np.ndarray           # f32 [M, K]
    B: np.ndarray           # f32 [K, N], unrounded
    profile: str = "normal"
    promoted: bool = True
    b_layout: str = "rows"

    def reference(self):
        """(float64 [M, N], bound [M, N]) over the operands as the kernel rounds them"""
        with np.errstate(over="ignore", invalid="ignore"):
            A = (self.A.astype(f16) if self.promoted and self.M > 1 else self.A).astype(f64)
            B = (self.B.astype(f16) if self.promoted else self.B).astype(f64)
            if self.profile == "overflow":  # term by term: inf - inf and 0 * inf as IEEE has them, whatever a BLAS would do
                want = np.stack([(A[m][:, None] * B).sum(axis=0) for m in range(self.M)])
                bound = np.stack([(np.abs(A[m])[:, None] * np.abs(B)).sum(axis=0) for m in range(self.M)])
                return want, bound
            return A @ B, np.abs(A) @ np.abs(B)

    def written(self):
        """indices of the dst buffer the matmul writes, [M, N]"""
        return self.d_off + np.arange(self.M)[:, None] * self.d_rs + np.arange(self.N)[None, :]


@dataclass
class Case:
    name: str
    cut: str                 # what the case is there for
    prog: DeviceProgram
    mats: list
    images: dict             # buffer -> its f32 image before the program runs (uploads; zero without one)
    launches: list           # [(op_lo, op_hi)] the plan text must show
    routes: dict             # first op of an f16 launch -> Route
    forced: Optional[str] = None     # key of FORCED, None: default switches
    nt: bool = False
    exec_inputs: list = field(default_factory=list)   # uploads at execution time (a B without an initial upload)
    expect: dict = field(default_factory=dict)        # declared facts of the cut: waves, trips, live_last, R, tiles, padded_rows, grid_y, CG
    solo_equal: bool = False         # every checked output must equal, bit for bit, the same matmul in a program of its own
    same_rows: list = field(default_factory=list)     # [(mat i, mat j, rows)]: the first `rows` rows of both must be bit-equal
    zero_ops: list = field(default_factory=list)      # [(buffer, n)]: outputs that must be exactly zero (the filler's)

    @property
    def env(self):
        return FORCED[self.forced] if self.forced else {}

    def promoted_case(self):
        return all(m.promoted for m in self.mats)


class _P:
    """program builder: poisoned operand buffers, sentinel outputs, matmul ops"""

    def __init__(self, name):
        self.rng = np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 32))
        self.sizes, self.images, self.ops, self.mats, self.qw, self.no_upload = [], {}, [], [], [], set()

    def buf(self, image, upload=True):
        image = np.ascontiguousarray(image, f32).ravel()
        self.sizes.append(image.size)
        self.images[len(self.sizes) - 1] = image
        if not upload:
            self.no_upload.add(len(self.sizes) - 1)
        return len(self.sizes) - 1

    def a_rows(self, A, a_off=4, pad=4, tail=5, rs=None):
        """A [M, K] as rows of stride K + pad behind a_off, NaN everywhere else"""
        M, K = A.shape
        rs = rs or K + pad
        img = np.full(a_off + (M - 1) * rs + K + pad + tail, np.nan, f32)
        for m in range(M):
            img[a_off + m * rs:][:K] = A[m]
        return self.buf(img), a_off, rs

    def b_image(self, B, layout="rows", b_off=7, tail=3):
        """-> (image, b_off, b_rs, b_cs). rows: [K][N] dense; wide: b_rs = N + 5 with NaN gaps; kcontig: b_rs = 1, b_cs = K + 3"""
        K, N = B.shape
        rs, cs = {"rows": (N, 1), "wide": (N + 5, 1), "kcontig": (1, K + 3)}[layout]
        img = np.full(b_off + (K - 1) * rs + (N - 1) * cs + 1 + tail, np.nan, f32)
        img[b_off + np.arange(K)[:, None] * rs + np.arange(N)[None, :] * cs] = B
        return img, b_off, rs, cs

    def dst(self, M, N, d_off=1, pad=3, tail=6):
        rs = N + pad
        return self.buf(np.full(d_off + (M - 1) * rs + N + tail, SENTINEL, f32)), d_off, rs

    def mat(self, M, K, N, profile="normal", a=None, b=None, d=None, a_off=4, b_layout="rows", values=None, promoted=True, a_cs=1):
        """one matmul op; a = (buffer, offset, rs, A) / b = (buffer, offset, rs, cs, B) / d = (buffer, offset, rs) reuse operands"""
        A, B = values if values else make_values(profile, self.rng, M, K, N)
        if a is not None:
            A = a[3]
        if b is not None:
            B = b[4]
        if a is None:
            a = (*self.a_rows(A, a_off=a_off), A)
        if b is None:
            img, b_off, b_rs, b_cs = self.b_image(B, b_layout)
            b = (self.buf(img), b_off, b_rs, b_cs, B)
        if d is None:
            d = self.dst(M, N)
        g = MatMulGeometry(M=M, N=N, K=K, a_row_stride=a[2], a_col_stride=a_cs, b_row_stride=b[2], b_col_stride=b[3],
                           a_offset=a[1], b_offset=b[1], dst_offset=d[1], dst_row_stride=d[2])
        self.ops.append(DeviceOp.matmul(d[0], a[0], b[0], g))
        m = Mat(len(self.ops) - 1, M, K, N, a[0], a[1], a[2], a_cs, b[0], d[0], d[1], d[2], np.ascontiguousarray(A[:M, :K]), B, profile, promoted, b_layout)
        self.mats.append(m)
        return m, a, b, d

    def program(self):
        ups = [ProgramIO(i, img) for i, img in self.images.items() if i not in self.no_upload]
        return DeviceProgram(ops=list(self.ops), buffer_sizes=list(self.sizes), initial_uploads=ups, qweights=list(self.qw))

    def case(self, name, cut, forced=None, **kw):
        prog = self.program()
        env = FORCED[forced] if forced else {}
        nt = stream_nt(prog)
        weights = promoted(prog)
        for m in self.mats:
            assert (m.b_buf in weights) == m.promoted, (name, m.op)
        routes = {}
        for L in plan(prog, env):
            if L.kind == "f16":
                g = prog.ops[L.lo].geom
                routes[L.lo] = route(g.M, g.K, [prog.ops[t].geom.N for t in L.parts], g.a_offset % 4 == 0, g.a_row_stride, nt, env)
        return Case(name, cut, prog, list(self.mats), dict(self.images), joins(prog, env), routes, forced, nt, **kw)


# cuts declared by hand; tests/test_dense_f16_cases_host.py holds route() to them
MV_CUTS = {  # K -> (waves, steps, live chunks of the last step): step = 8 chunks per wave, at most 4 waves
    1: (1, 1, 1), 31: (1, 1, 1), 32: (1, 1, 1), 33: (1, 1, 2), 100: (1, 1, 4), 256: (1, 1, 8), 288: (2, 1, 9), 1024: (4, 1, 32),
    1056: (4, 2, 1), 2080: (4, 3, 1), 1030: (4, 2, 1)}
M_CUTS = {  # M -> (R, m-tiles of the A operand, padded rows, grid.y)
    2: (1, 1, 14, 1), 16: (1, 1, 0, 1), 17: (2, 2, 15, 1), 32: (2, 2, 0, 1), 33: (4, 4, 31, 1), 48: (4, 4, 16, 1), 64: (4, 4, 0, 1),
    65: (8, 8, 63, 1), 80: (8, 8, 48, 1), 128: (8, 8, 0, 1), 129: (8, 16, 127, 2)}
T2_CUTS = {  # (R class, K) -> (waves, trips, live chunks of the last trip): DEPTH 4 / 3 / 2 chunks per wave and trip
    2: {3: (1, 1, 1), 32: (1, 1, 1), 37: (2, 1, 2), 256: (8, 1, 8), 288: (8, 1, 9), 1024: (8, 1, 32), 1056: (8, 2, 1)},
    4: {32: (1, 1, 1), 37: (2, 1, 2), 768: (8, 1, 24), 800: (8, 2, 1)},
    8: {32: (1, 1, 1), 37: (2, 1, 2), 512: (8, 1, 16), 544: (8, 2, 1)}}
PAST_TRIP = {1: 1056, 2: 1056, 4: 800, 8: 544}  # one chunk past the loop trip, per R

_BUILDERS = {}


def _single(name, cut, M, K, N, profile="normal", a_off=4, b_layout="rows", forced=None, expect=None):
    p = _P(name)
    p.mat(M, K, N, profile, a_off=a_off, b_layout=b_layout)
    return p.case(name, cut, forced, expect=expect or {})


def _mv_expect(K):
    w, t, l = MV_CUTS[K]
    return dict(waves=w, trips=t, live_last=l, R=0, grid_y=1, CG=1)


def _t2_expect(M, K, CG=1):
    R, tiles, pad, gy = M_CUTS[M]
    w, t, l = T2_CUTS[2 if R <= 2 else R][K]
    return dict(waves=w, trips=t, live_last=l, R=R, tiles=tiles, padded_rows=pad, grid_y=gy, CG=CG)


def _add(name, fn):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = fn


# mat-vec, M = 1: every K at N = 16 (normal) and N = 48 (f16_edges); zero columns and overflows at the ragged K
for _K in (1, 31, 32, 33, 100, 256, 288, 1024, 1056, 2080):
    for _N, _prof in ((16, "normal"), (48, "f16_edges")):
        _add(f"mv_k{_K}_n{_N}_{_prof}", lambda n, K=_K, N=_N, pr=_prof: _single(n, f"mat-vec K {K}", 1, K, N, pr, expect=_mv_expect(K)))
for _K, _prof in ((100, "zero_row"), (1056, "zero_row"), (33, "overflow"), (288, "overflow"), (1056, "overflow"), (2080, "overflow")):
    _add(f"mv_k{_K}_n16_{_prof}", lambda n, K=_K, pr=_prof: _single(n, f"mat-vec K {K}, {pr}", 1, K, 16, pr, expect=_mv_expect(K)))
# the scalar-load form: K % 4 != 0; A at offset 1
for _K, _off, _prof in ((1030, 4, "normal"), (1030, 4, "f16_edges"), (1030, 4, "overflow"), (1056, 1, "normal"), (1056, 1, "f16_edges")):
    _add(f"mv_scalar_k{_K}_off{_off}_{_prof}", lambda n, K=_K, o=_off, pr=_prof: _single(n, f"mat-vec XVEC = false, K {K}, A offset {o}", 1, K, 48, pr,
                                                                                 a_off=o, expect=_mv_expect(K)))
_add("mv_b_wide", lambda n: _single(n, "b_rs > N, NaN in the gaps", 1, 288, 16, b_layout="wide", expect=_mv_expect(288)))
_add("mv_b_kcontig", lambda n: _single(n, "K-contiguous B: b_rs = 1, b_cs = K + 3", 1, 288, 48, b_layout="kcontig", expect=_mv_expect(288)))

# tile kernel: the K x M grid at N = 32
for _M, (_R, _, _, _) in M_CUTS.items():
    for _K in (k for k in T2_CUTS[2 if _R <= 2 else _R] if k != 3):
        _add(f"t2_m{_M}_k{_K}", lambda n, M=_M, K=_K: _single(n, f"tile kernel M {M}, K {K}", M, K, 32, expect=_t2_expect(M, K)))
_add("t2_m2_k3_n16", lambda n: _single(n, "K = 3, N = 16: one chunk, one column group", 2, 3, 16, expect=_t2_expect(2, 3)))
_add("t2_m16_k37_n16", lambda n: _single(n, "N = 16: one column group", 16, 37, 16, expect=_t2_expect(16, 37)))
for _M in (16, 17, 32, 48, 64, 65, 128, 129):
    _K = PAST_TRIP[M_CUTS[_M][0]]
    for _prof in ("f16_edges", "overflow") + (("zero_row",) if _M in (17, 48, 129) else ()):
        _add(f"t2_m{_M}_k{_K}_{_prof}", lambda n, M=_M, K=_K, pr=_prof: _single(n, f"tile kernel M {M}, K {K}, {pr}", M, K, 32, pr, expect=_t2_expect(M, K)))
_add("t2_m32_k288_overflow", lambda n: _single(n, "overflow in chunk 8, the one chunk of wave 0's second slot", 32, 288, 32, "overflow", expect=_t2_expect(32, 288)))
_add("t2_b_wide", lambda n: _single(n, "b_rs > N, NaN in the gaps", 17, 288, 32, b_layout="wide", expect=_t2_expect(17, 288)))
_add("t2_b_kcontig", lambda n: _single(n, "K-contiguous B", 33, 37, 32, b_layout="kcontig", expect=_t2_expect(33, 37)))


def _rows_pair(name, M_small, M_big, K):
    """two matmuls over the same A rows and the same weight, M_small and M_big rows: same (R, CG, waves) class, so the rows
    they share must come out bit-equal"""
    p = _P(name)
    _, a, b, _ = p.mat(M_big, K, 32, "f16_edges")
    p.mat(M_small, K, 32, "f16_edges", a=a, b=b)
    return p.case(name, f"rows do not depend on the other rows of the launch: M {M_small} against {M_big}", same_rows=[(0, 1, M_small)])


_add("t2_rows_17_32", lambda n: _rows_pair(n, 17, 32, 1056))
_add("t2_rows_65_128", lambda n: _rows_pair(n, 65, 128, 544))

# CG = 2: >= 1280 column groups, every part an even count
_add("t2_cg2_m32", lambda n: _single(n, "CG = 2 at R = 2; pack_f16_kernel's second grid-stride pass", 32, 256, 20480, "f16_edges", expect=_t2_expect(32, 256, 2)))
_add("t2_cg2_m16", lambda n: _single(n, "CG = 2 at R = 1", 16, 256, 20480, "f16_edges", expect=_t2_expect(16, 256, 2)))
_add("t2_m16_k64_n24576_f16_edges", lambda n: _single(n, "subnormal operands next to products 2^16 times larger, enough outputs to meet them: the matrix cores' finding",
                                                      16, 64, 24576, "f16_edges", expect=dict(R=1, CG=2, waves=2, trips=1, live_last=2)))
_add("t2_cg2_refused_odd", lambda n: _single(n, "1281 column groups, an odd count: CG = 1", 32, 256, 20496, expect=_t2_expect(32, 256, 1)))


def _group(name, cut, Ns, M=32, K=256, profile="normal", **kw):
    p = _P(name)
    _, a, _, _ = p.mat(M, K, Ns[0], profile)
    for N in Ns[1:]:
        p.mat(M, K, N, profile, a=a)
    return p.case(name, cut, solo_equal=True, **kw)


_add("t2_cg2_group", lambda n: _group(n, "a group (10240, 10240) at CG = 2: block_begin of part 1 is 320", (10240, 10240), expect=dict(CG=2)))

# plan level, M = 32, K = 256
_add("plan_three", lambda n: _group(n, "three matmuls over the same rows: one launch", (32, 32, 32)))
_add("plan_four", lambda n: _group(n, "four: a launch of three, then one that reuses the packed A", (32, 32, 32, 32)))
_add("plan_parts_n", lambda n: _group(n, "three parts of different N: block_begin 2 and 3", (32, 16, 48), profile="f16_edges"))


def _plan_overlap(name):
    """the second dst interleaves with the first's rows (its span overlaps, its elements do not): not joined, A reused"""
    p = _P(name)
    N, M, K = 32, 32, 256
    buf = p.buf(np.full(1 + (M - 1) * (2 * N + 5) + 2 * N + 9, SENTINEL, f32))
    _, a, _, _ = p.mat(M, K, N, d=(buf, 1, 2 * N + 5))
    p.mat(M, K, N, a=a, d=(buf, 1 + N + 2, 2 * N + 5))
    return p.case(name, "a dst whose span overlaps the first's: a launch of its own that reuses A", solo_equal=True)


def _plan_other_k(name):
    p = _P(name)
    _, a, _, _ = p.mat(32, 256, 32)
    p.mat(32, 224, 32, a=(a[0], a[1], a[2], a[3][:, :224]))
    return p.case(name, "the same rows at another K: not joined, packed again", solo_equal=True)


def _plan_other_rs(name):
    p = _P(name)
    M, K = 32, 256
    A = p.rng.standard_normal((2 * M, K)).astype(f32)
    A[M + 1::2] = np.nan  # the rows neither matmul reads
    buf, off, rs = p.a_rows(A)
    p.mat(M, K, 32, a=(buf, off, rs, A[:M]))
    p.mat(M, K, 32, a=(buf, off, 2 * rs, A[::2]))
    return p.case(name, "the same first row at another a_rs: not joined, packed again", solo_equal=True)


def _plan_q4_between(name):
    """f16, a Q4_0 qmatmul over the same rows (its split takes the shared scratch), f16 again: the third packs its own A"""
    p = _P(name)
    M, K, N = 32, 256, 32
    _, a, _, _ = p.mat(M, K, N)
    data = p.rng.integers(-8, 8, K * 64).astype(np.int8)
    scales = (p.rng.random(K * 64 // 32).astype(f16) * 0.05 + 0.001).astype(f32)  # f16-exact (tests/handover_cases.py consume)
    p.qw.append(QuantizedWeightUpload(data, scales, K, 64, 32))
    y = p.buf(np.full(M * 64 + 8, SENTINEL, f32))
    p.ops.append(DeviceOp.qmatmul(y, a[0], 0, M, 64, K, input_offset=a[1], input_row_stride=a[2]))
    p.mat(M, K, N, a=a)
    return p.case(name, "the quantized split owns the scratch in between: split_kind, split_pos + 1 == pos", solo_equal=True)


_add("plan_dst_overlap", _plan_overlap)
_add("plan_other_k", _plan_other_k)
_add("plan_other_a_rs", _plan_other_rs)
_add("plan_q4_between", _plan_q4_between)


def _nt(name):
    """every NT instantiation in one program: a zero filler weight of exactly 192 MiB packed (one 4096 x 24576 buffer, the
    smallest that crosses the threshold; only its first 64 words are uploaded, the staging image is zero behind them) next to
    small checked matmuls. a[0] = 0 keeps the filler's output exactly zero."""
    p = _P(name)
    fa = p.rng.standard_normal(FILLER_K).astype(f32)
    fa[0] = 0
    fa_buf = p.buf(fa)
    p.sizes.append(FILLER_K * FILLER_N)
    fb = len(p.sizes) - 1
    p.images[fb] = p.rng.standard_normal(64).astype(f32)  # row 0, columns 0..63 (partial upload)
    fd = p.buf(np.full(FILLER_N + 4, SENTINEL, f32))
    p.ops.append(DeviceOp.matmul(fd, fa_buf, fb, MatMulGeometry(M=1, N=FILLER_N, K=FILLER_K, a_row_stride=FILLER_K, a_col_stride=1, b_row_stride=FILLER_N,
                                                                b_col_stride=1, a_offset=0, b_offset=0, dst_offset=0, dst_row_stride=FILLER_N)))
    for off in (4, 1):
        for prof in ("f16_edges", "overflow"):
            p.mat(1, 1056, 48, prof, a_off=off)
    for M in (16, 32, 64, 128):
        p.mat(M, 1056, 32, "f16_edges")
    for M in (32, 128):
        p.mat(M, 1056, 32, "overflow")
    _, _, b, _ = p.mat(32, 256, 20480, "f16_edges")
    p.mat(16, 256, 20480, "f16_edges", b=b)
    p.mat(129, 1056, 32)
    return p.case(name, "the NT forms: M = 1 aligned and offset 1, R = 1 / 2 / 4 / 8, CG = 2 at R = 1 / 2, and M = 129 falling back", solo_equal=True,
                  zero_ops=[(fd, FILLER_N)])


_add("nt_program", _nt)


# promotion refused, one clause of promoted() each, at M = 1 and M = 17: bit-equal to the program with the option off
def _refused(name, clause, M):
    p = _P(name)
    K, N = 256, 32
    kw = {}
    if clause == "no_upload":  # B arrives at execution time
        m, a, b, d = p.mat(M, K, N, promoted=False)
        p.no_upload.add(b[0])
        kw["exec_inputs"] = [b[0]]
    elif clause == "other_reader":  # an elementwise op reads B too
        m, a, b, d = p.mat(M, K, N, promoted=False)
        n = p.sizes[b[0]] - b[1] - 3
        sink = p.buf(np.full(n, SENTINEL, f32))
        p.ops.append(DeviceOp.elementwise("neg", sink, b[0], b[0], n, src0_offset=b[1], src1_offset=b[1]))
    elif clause == "two_geometries":  # a second matmul reads the same buffer from another offset, fewer k
        m, a, b, d = p.mat(M, K, N, promoted=False)
        p.mat(M, K - 32, N, a=(a[0], a[1], a[2], a[3][:, :K - 32]), b=(b[0], b[1] + 32 * N, b[2], b[3], b[4][32:]), promoted=False)
    elif clause == "written":  # an op writes B in front of the matmul: B = -S
        A, B = make_values("normal", p.rng, M, K, N)
        img, b_off, b_rs, b_cs = p.b_image(B)
        src = p.buf(-img)
        bb = p.buf(img * 0 + 3)
        p.ops.append(DeviceOp.elementwise("neg", bb, src, src, img.size))
        p.mat(M, K, N, b=(bb, b_off, b_rs, b_cs, B), values=(A, B), promoted=False)
    elif clause == "a_col_stride":  # A stored with a column stride of 2
        A, B = make_values("normal", p.rng, M, K, N)
        rs = 2 * K + 6
        img = np.full(4 + M * rs + 5, np.nan, f32)
        for r in range(M):
            img[4 + r * rs:][:2 * K:2] = A[r]
        p.mat(M, K, N, a=(p.buf(img), 4, rs, A), values=(A, B), promoted=False, a_cs=2)
    elif clause == "n_not_16":
        p.mat(M, K, 24, promoted=False)
    elif clause == "a_is_b":  # A rows and B in one buffer
        A, B = make_values("normal", p.rng, M, K, N)
        img, b_off, b_rs, b_cs = p.b_image(B)
        rs = K + 4
        rows = np.full(M * rs + 5, np.nan, f32)
        for r in range(M):
            rows[r * rs:][:K] = A[r]
        buf = p.buf(np.concatenate([img, rows]))
        p.mat(M, K, N, a=(buf, img.size, rs, A), b=(buf, b_off, b_rs, b_cs, B), values=(A, B), promoted=False)
    elif clause == "dst_is_b":  # the result goes behind B in B's own buffer
        A, B = make_values("normal", p.rng, M, K, N)
        img, b_off, b_rs, b_cs = p.b_image(B)
        d_rs = N + 3
        buf = p.buf(np.concatenate([img, np.full(1 + M * d_rs + 6, SENTINEL, f32)]))
        p.mat(M, K, N, b=(buf, b_off, b_rs, b_cs, B), d=(buf, img.size + 1, d_rs), values=(A, B), promoted=False)
    elif clause == "also_an_a":  # another matmul reads the buffer as its A rows
        m, a, b, d = p.mat(M, K, N, promoted=False)
        A2 = np.nan_to_num(p.images[b[0]][b[1]:][:2 * N].reshape(2, N))
        p.mat(2, N, 16, a=(b[0], b[1], N, A2), promoted=True)
    else:
        raise KeyError(clause)
    return p.case(name, f"promotion refused: {clause}", **kw)


REFUSED_CLAUSES = ("no_upload", "other_reader", "two_geometries", "written", "a_col_stride", "n_not_16", "a_is_b", "dst_is_b", "also_an_a")
for _c in REFUSED_CLAUSES:
    for _M in (1, 17):
        _add(f"refused_{_c}_m{_M}", lambda n, c=_c, M=_M: _refused(n, c, M))


# ── env-only forms: each table runs in a child process with FORCED[key] set ──────────────────────────────────────────────

STAGED_CUTS = {37: (1, 1, 2), 1024: (None, 1, 32), 1056: (None, 2, 1)}  # K -> (waves or by R, steps, live): R = 1 4 waves x 8, R = 2 8 waves x 4


def _staged_expect(M, K, G=1):
    w, t, l = STAGED_CUTS.get(K, (1, 1, cdiv(K, 32)))
    R = 2 if M > 16 else 1
    return dict(waves=w or (8 if R == 2 else 4), trips=t, live_last=l, R=R, grid_y=cdiv(M, 16 * R), CG=G)


for _M in (2, 16, 17, 32, 45):
    for _K in (37, 1024, 1056):
        _prof = {37: "normal", 1024: "f16_edges", 1056: "overflow"}[_K]
        _add(f"staged_m{_M}_k{_K}", lambda n, M=_M, K=_K, pr=_prof: _single(n, f"staged form M {M}, K {K}" + (", the 132 KB LDS path" if M > 16 and K >= 1024 else ""),
                                                                             M, K, 32, pr, forced="staged", expect=_staged_expect(M, K)))
    _add(f"staged_m{_M}_k1056_off1", lambda n, M=_M: _single(n, f"staged form XVEC = false, M {M}", M, 1056, 32, "f16_edges", a_off=1, forced="staged",
                                                             expect=_staged_expect(M, 1056)))
for _M in (16, 32):
    for _off in (4, 1):
        _add(f"staged_g2_m{_M}_off{_off}", lambda n, M=_M, o=_off: _single(n, f"staged form G = 2, M {M}, A offset {o}", M, 64, 24576, "f16_edges", a_off=o, forced="staged",
                                                                           expect=_staged_expect(M, 64, 2)))
for _M in (16, 32):
    for _K, _prof in ((37, "normal"), (800, "f16_edges"), (800, "overflow")):
        _add(f"cg4_m{_M}_k{_K}_{_prof}", lambda n, M=_M, K=_K, pr=_prof: _single(n, f"CG = 4 (DEPTH 3), M {M}, K {K}", M, K, 64, pr, forced="cg4",
                                                                                expect=dict(CG=4, R=M_CUTS[M][0], trips=cdiv(cdiv(K, 32), 24), waves=min(cdiv(K, 32), 8))))
for _M, _gy in ((45, 2), (129, 5)):
    for _prof in ("f16_edges", "overflow"):
        _add(f"narrow3_m{_M}_{_prof}", lambda n, M=_M, gy=_gy, pr=_prof: _single(n, f"R = 2 over {gy} row groups, 3 waves", M, 1056, 32, pr, forced="narrow3",
                                                                                 expect=dict(R=2, waves=3, trips=3, live_last=9, grid_y=gy, CG=1)))

CASE_NAMES = tuple(_BUILDERS)
_FORCED_OF = {n: next((k for k in FORCED if n.startswith(k + "_")), None) for n in CASE_NAMES}
DEFAULT_CASES = tuple(n for n in CASE_NAMES if _FORCED_OF[n] is None)
_cache = {}


def forced_cases(key):
    return tuple(n for n in CASE_NAMES if _FORCED_OF[n] == key)


def build_case(name) -> Case:
    """built once per process and shared: nothing may modify a case"""
    if name not in _cache:
        _cache[name] = _BUILDERS[name](name)
    return _cache[name]


# the instantiations default switches can reach (launch_dense_f16 at M = 1, launch_dense_f16_tile2), and the env-only ones
DEFAULT_INSTANTIATIONS = frozenset(
    [f"dense_f16_kernel<0, {x}, 1, {n}>" for x in ("true", "false") for n in ("true", "false")] +
    [f"dense_f16_tile2_kernel<{R}, {n}, {cg}>" for R in (1, 2) for cg in (1, 2) for n in ("true", "false")] +
    [f"dense_f16_tile2_kernel<{R}, {n}, 1>" for R in (4, 8) for n in ("true", "false")])
FORCED_INSTANTIATIONS = {
    "staged": frozenset(f"dense_f16_kernel<{R}, {x}, {G}, false>" for R in (1, 2) for x in ("true", "false") for G in (1, 2)),
    "cg4": frozenset(f"dense_f16_tile2_kernel<{R}, false, 4>" for R in (1, 2)),
    "narrow3": frozenset(["dense_f16_tile2_kernel<2, false, 1>"])}


# ── running a case ─────────────────────────────────────────────────────────────────────────────────────────────────────

def solo_program(case, mat):
    """the matmul alone, in a program of its own, over the same operand images"""
    op = case.prog.ops[mat.op]
    bufs = [mat.a_buf, mat.b_buf, mat.d_buf]
    idx = {b: i for i, b in enumerate(dict.fromkeys(bufs))}
    return DeviceProgram(ops=[op.with_(dst=idx[mat.d_buf], a=idx[mat.a_buf], b=idx[mat.b_buf])], buffer_sizes=[case.prog.buffer_sizes[b] for b in idx],
                         initial_uploads=[ProgramIO(i, case.images[b]) for b, i in idx.items()]), idx[mat.d_buf]


def run(be, prog, out_bufs, exec_inputs=(), images=None, executes=1, plan_text=False):
    """compile, execute `executes` times, download the buffers: ({buffer: [f32 image per execution]}, plan text or None)"""
    h = be.compileProgram(prog)
    if not h:
        raise RuntimeError("compile failed")
    try:
        text = be.planText(h) if plan_text else None
        got = {b: [] for b in out_bufs}
        for _ in range(executes):
            outs = {b: np.zeros(prog.buffer_sizes[b], f32) for b in out_bufs}
            be.executeProgram(h, [ProgramIO(b, images[b]) for b in exec_inputs], [ProgramIO(b, o) for b, o in outs.items()])
            for b, o in outs.items():
                got[b].append(o)
    finally:
        be.freeProgram(h)
    return got, text


DOT_RATIO = 2.0 ** -15   # a dot mixes magnitudes when a subnormal-operand product is at most this fraction of its largest product
MAX_SLACK_OUTPUTS = 64   # outputs of one matmul that may need the term at all (measured: about twenty of 393216)


def subnormal_slack(m, r, n):
    """What output (r, n) of an M > 1 matmul is allowed on top of the contract on the matrix cores. A 32-k dot of the instruction
    (k in [32 c, 32 c + 32)) mixes magnitudes when it holds a product with a nonzero f16-subnormal operand that is no larger than
    DOT_RATIO times the dot's largest product; every subnormal operand of such a dot then counts with the issue's term,
    2^-14 * |other operand|. Zero where no dot of the output mixes magnitudes."""
    with np.errstate(over="ignore"):
        a, b = np.abs(m.A[r].astype(f16).astype(f64)), np.abs(m.B[:, n].astype(f16).astype(f64))
    pad = -len(a) % 32
    a, b = np.pad(a, (0, pad)).reshape(-1, 32), np.pad(b, (0, pad)).reshape(-1, 32)
    p = a * b
    sub_a, sub_b = (p > 0) & (a < 2.0 ** -14), (p > 0) & (b < 2.0 ** -14)
    mixed = ((sub_a | sub_b) & (p <= DOT_RATIO * p.max(axis=1, keepdims=True))).any(axis=1, keepdims=True)
    return float(2.0 ** -14 * (np.where(mixed & sub_a, b, 0).sum() + np.where(mixed & sub_b, a, 0).sum()))


def check_mat(case, m, out, what="", matrix_cores=False):
    """one matmul's output buffer image against float64, every output compared: -> (worst error / bound, worst error over the
    contract bar alone). matrix_cores: the run is the device's; an output of an M > 1 form on f16_edges that misses the contract
    is then held to contract + subnormal_slack, unless it lies in a subnormal-only column (those stay on the contract alone),
    and at most MAX_SLACK_OUTPUTS outputs of a matmul may need that."""
    want, bound = m.reference()
    got = out[m.written()].astype(f64)
    where = f"{case.name} op {m.op}{what}"
    if m.profile == "overflow":
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{where}: NaN at {np.argwhere(np.isnan(got) != np.isnan(want))[:6].tolist()}"
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(want[inf])), f"{where}: inf pattern differs"
        fin = np.isfinite(want)
        assert fin.any() and not fin.all(), where
    else:
        assert np.isfinite(want).all() and np.isfinite(bound).all(), where
        fin = np.ones(want.shape, bool)
    assert np.isfinite(got[fin]).all(), f"{where}: non-finite output where float64 is finite"
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    contract = TOL * np.where(fin, bound, 0) + FLOOR
    bar = contract.copy()
    miss = np.argwhere((err > bar) & fin)
    if len(miss) and matrix_cores and m.promoted and m.M > 1 and m.profile == "f16_edges":
        assert len(miss) <= MAX_SLACK_OUTPUTS, f"{where}: {len(miss)} outputs miss the contract, first at {miss[:6].tolist()}"
        only_sub = set(subnormal_only_columns(m.N))
        for r, n in miss:
            if n not in only_sub:
                bar[r, n] += subnormal_slack(m, r, n)
    ratio = float(np.max(err[fin] / bar[fin]))
    assert ratio <= 1.0, f"{where}: {ratio:.3g} of the bar at {np.argwhere((err > bar) & fin)[:6].tolist()}"
    if m.profile == "zero_row":
        assert np.all(got[:, 3] == 0), where
        if m.M > 1:
            assert np.all(got[min(5, m.M - 1)] == 0), where
    return float(np.max(err[fin] / np.maximum(bound[fin], FLOOR))), float(np.max(err[fin] / contract[fin]))


def untouched(case, bufs):
    """every word no checked matmul writes still holds its image (the sentinel in a dst of its own)"""
    for b, out in bufs.items():
        keep = np.ones(out.size, bool)
        for m in case.mats:
            if m.d_buf == b:
                keep[m.written().ravel()] = False
        for zb, n in case.zero_ops:
            if zb == b:
                keep[:n] = False
        img = case.images[b]
        assert np.array_equal(out[keep].view(np.uint32), img[keep].view(np.uint32)), f"{case.name}: buffer {b} written outside its matmul's outputs"
