"""Case table for the A-operand hand-over from a producing launch to an M > 1 matmul (zgml_amd/csrc/plan.hip make_single,
SplitHook): a row chain, an elementwise chain or the attention tile kernel writes the next matmul's A operand (bf16 pieces for
a Q4_0 qmatmul, f16 halves for an f16-promoted dense matmul) next to its f32 output, and the matmul skips its own split / pack
launch. No GPU and no HIP library here: programs, which launch should carry the plan text's tag, and float64 numpy references.

A case holds one DeviceProgram and one or more steps (step 0: as compiled; further steps: a refresh before the execution).
Per step: the float64 reference of the producer's output X as the consumers see it (after any writer in between), the op ranges
of the launches that must carry the tag (every other launch must not; None: not asserted), and the consumers, each checked
against a float64 reference computed from the f32 X the device (or the oracle) really produced:
  Q4 : X @ dequant(W) in float64, bound |X| @ |W| (tests/test_hip_qmatvec.py::bound)
  f16: X and B each rounded to np.float16, products and sums in float64, bound |X| @ |B|
at |delta| <= 2e-5 * bound, the contract bar of tests/test_hip_qmatvec.py and tests/test_hip_dense_f16.py.

Arming rules the table restates case by case (plan.hip): a Q4 consumer arms for M % 16 == 0, K % 128 == 0 and dense rows; an
f16 consumer for M % 16 == 0, K % 32 == 0, dense rows and an A operand without padding tiles (dense_f16_a_unpadded: the
m-tiles divide by the 1 / 2 / 4 / 8 tiles a workgroup carries at M <= 16 / <= 32 / <= 64 / above, so M = 48 and M = 80 pad).
A producer is armed only when no op between its last member and the matmul writes the matmul's input rows."""
from dataclasses import dataclass, field, replace
from typing import Callable, Optional

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, FusedEwStep, MatMulGeometry, ProgramIO, QuantizedWeightUpload

f32, f64 = np.float32, np.float64
TAG = "writes-A-operand"
TOL = 2e-5        # |Y - ref| <= TOL * bound
SENTINEL = -7.0
N_OUT = 64
BARS = {"rms": dict(atol=1e-5, rtol=1e-5), "silu": dict(atol=1e-6, rtol=1e-5), "attn": dict(atol=2e-5, rtol=0.0)}


@dataclass
class Consumer:
    kind: str                 # "q4" | "f16"
    op: int                   # index of its op in the program
    M: int
    K: int
    N: int
    x_buf: int
    x_off: int
    x_rs: int
    y_buf: int
    weight: object            # QuantizedWeightUpload | (buffer index, f32 [K, N])
    x_of: Optional[Callable] = None  # bufs -> f32 [M, K]: the rows it read, where a later op overwrote them
    y_tail: int = 0           # sentinel elements behind the M x N result

    def x(self, bufs):
        if self.x_of:
            return np.ascontiguousarray(self.x_of(bufs), f32)
        b = bufs[self.x_buf]
        return np.stack([b[self.x_off + m * self.x_rs:][:self.K] for m in range(self.M)])

    def reference(self, x32):
        """(float64 Y [M, N], bound [M, N]) from the f32 rows the matmul read"""
        if self.kind == "q4":
            w = self.weight
            W = (w.data.astype(f64) * np.repeat(w.scales.astype(f64), w.block_size)[:w.data.size]).reshape(self.K, self.N)
            X = x32.astype(f64)
        else:
            W = self.weight[1].astype(np.float16).astype(f64)
            X = x32.astype(np.float16).astype(f64)
        return X @ W, np.abs(X) @ np.abs(W)


@dataclass
class Step:
    ops: Optional[list]       # None: the program as compiled; else the op list of a static refresh
    x_ref: np.ndarray         # float64 [rows, cols] of the region (Case.x_buf, x_off)
    tagged: Optional[set]     # {(op_lo, op_hi)} of the launches that carry TAG; None: not asserted
    consumers: list


@dataclass
class Case:
    name: str
    kind: str                 # consumer kind the case is about ("q4" | "f16" | "mixed"): f16 and mixed compile with promotion on
    prog: DeviceProgram
    steps: list
    bars: dict
    x_buf: int
    x_off: int
    group: Optional[tuple] = None    # (op_lo, op_hi, n_ops): a launch that must exist
    downloads: list = field(default_factory=list)
    control: bool = False

    @property
    def f16(self):
        return self.kind != "q4"


class _B:
    """program builder: buffers with their uploads, weights, ops"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.sizes, self.ups, self.ops, self.qw, self.vals = [], [], [], [], {}

    def buf(self, a):
        a = np.ascontiguousarray(a, f32).ravel()
        self.sizes.append(a.size)
        self.ups.append(ProgramIO(len(self.sizes) - 1, a))
        self.vals[len(self.sizes) - 1] = a
        return len(self.sizes) - 1

    def uni(self, n, lo=-1.0, hi=1.0):
        return self.buf(self.rng.uniform(lo, hi, n))

    def op(self, o):
        self.ops.append(o)
        return len(self.ops) - 1

    def consume(self, kind, x_buf, x_off, M, K, N=N_OUT, x_rs=None, tail=8, x_of=None):
        x_rs = x_rs or K
        y = self.buf(np.full(M * N + tail, SENTINEL))
        if kind == "q4":  # Q4_0 with f16-exact scales (tests/test_hip_qmatvec.py::_q4_weight)
            data = self.rng.integers(-8, 8, K * N).astype(np.int8)
            scales = (self.rng.random(K * N // 32).astype(np.float16) * 0.05 + 0.001).astype(f32)
            w = QuantizedWeightUpload(data, scales, K, N, 32)
            self.qw.append(w)
            i = self.op(DeviceOp.qmatmul(y, x_buf, len(self.qw) - 1, M, N, K, input_offset=x_off, input_row_stride=x_rs))
        else:  # an uploaded B only matmuls read: promoted (tests/test_hip_dense_f16.py)
            bv = (self.rng.standard_normal(K * N) * 0.05).astype(f32)
            bb = self.buf(bv)
            w = (bb, bv.reshape(K, N))
            i = self.op(DeviceOp.matmul(y, x_buf, bb, MatMulGeometry(M=M, N=N, K=K, a_row_stride=x_rs, a_col_stride=1, b_row_stride=N,
                                                                     b_col_stride=1, a_offset=x_off, b_offset=0, dst_offset=0, dst_row_stride=N)))
        return Consumer(kind, i, M, K, N, x_buf, x_off, x_rs, y, w, x_of, tail)

    def program(self, ops=None):
        return DeviceProgram(ops=list(self.ops if ops is None else ops), buffer_sizes=list(self.sizes), initial_uploads=list(self.ups),
                             qweights=list(self.qw))


# ── float64 references of the producers ────────────────────────────────────────────────────────────────────────────────

def rms64(s, eps):
    s = s.astype(f64)
    return s / np.sqrt((s * s).mean(axis=1, keepdims=True) + eps)


def silu_up64(g, u):
    g, u = g.astype(f64), u.astype(f64)
    return g / (1.0 + np.exp(-g)) * u


def softmax64(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def attention64(q, k, v, mask, scale):
    """q [sq, dh], k / v [skv, dh], mask [sq, skv] of 0 / -inf (every query keeps a key)"""
    return softmax64(scale * (q.astype(f64) @ k.astype(f64).T) + mask.astype(f64)) @ v.astype(f64)


# ── producers ──────────────────────────────────────────────────────────────────────────────────────────────────────────

def _row_chain(b, M, K, form="norm_mul", eps=1e-5, x_rows=None):
    """[add ->] rmsnorm [-> mul] over M dense rows of K columns. Returns (X buffer, float64 X [M, K], (first, last) member op,
    index of the rmsnorm op). `x_rows` > M: X has further uploaded rows behind the chain's."""
    n = M * K
    if form.startswith("add"):
        a0, a1 = b.uni(n), b.uni(n)
        s = b.buf(np.zeros(n))
        first = b.op(DeviceOp.elementwise("add", s, a0, a1, n))
        sv = b.vals[a0] + b.vals[a1]  # f32 sum, as the device forms it
    else:
        s = b.uni(n)
        first, sv = None, b.vals[s]
    x_n = (x_rows or M) * K
    norm_is_x = form.endswith("norm")
    nrm = b.uni(x_n) if norm_is_x else b.buf(np.zeros(n))
    i_norm = b.op(DeviceOp.rmsnorm(nrm, s, M, K, eps))
    first = i_norm if first is None else first
    ref = rms64(sv.reshape(M, K), eps)
    if norm_is_x:
        return nrm, ref, (first, i_norm), i_norm
    g = b.uni(n, 0.5, 1.5)
    x = b.uni(x_n)
    last = b.op(DeviceOp.elementwise("mul", x, nrm, g, n))
    return x, ref * b.vals[g].reshape(M, K).astype(f64), (first, last), i_norm


def _silu_chain(b, n, x_off=0, x_pad=0):
    """SiLU(gate) * up as the LLaMA lowering emits it: [neg, exp] -> [add 1, recip, mul gate] -> mul up, X at x_off of its buffer"""
    g, u, one = b.uni(n), b.uni(n), b.buf(np.ones(n))
    exp_neg, silu = b.buf(np.zeros(n)), b.buf(np.zeros(n))
    x = b.uni(x_off + n + x_pad)
    first = b.op(DeviceOp.fused_elementwise([FusedEwStep("neg"), FusedEwStep("exp")], n, exp_neg, g))
    b.op(DeviceOp.fused_elementwise([FusedEwStep("add", False, one, 0), FusedEwStep("recip"), FusedEwStep("mul", True, g, 0)], n, silu, exp_neg))
    last = b.op(DeviceOp.elementwise("mul", x, silu, u, n, dst_offset=x_off))
    return x, silu_up64(b.vals[g], b.vals[u]), (first, last)


def _attention(b, dh, n_heads, sq, skv=40):
    """per head: attention over its own q / k / v rows, then the row store into columns h * dh of one [sq x n_heads * dh] matrix"""
    K = dh * n_heads
    q, k, v = b.uni(n_heads * sq * dh), b.uni(n_heads * skv * dh), b.uni(n_heads * skv * dh)
    mask = np.where(np.arange(skv)[None, :] <= (skv - sq + np.arange(sq))[:, None], 0.0, -np.inf).astype(f32)  # causal-style
    mb, ao, x = b.buf(mask), b.buf(np.zeros(n_heads * sq * dh)), b.uni(sq * K)
    scale = dh ** -0.5
    for h in range(n_heads):
        b.op(DeviceOp.attention(ao, q, k, v, mb, True, dh, sq, skv, scale, h * sq * dh, h * skv * dh, h * skv * dh, 0, h * sq * dh,
                                1, dh, 1, dh, 1, dh, 1, skv, 1, dh))
    for h in range(n_heads):
        b.op(DeviceOp.slice_assign(x, ao, dh, sq, h * dh, h * dh, 1, K, h * sq * dh, 1, dh, 0))
    ref = np.concatenate([attention64(b.vals[q][h * sq * dh:][:sq * dh].reshape(sq, dh), b.vals[k][h * skv * dh:][:skv * dh].reshape(skv, dh),
                                      b.vals[v][h * skv * dh:][:skv * dh].reshape(skv, dh), mask, scale) for h in range(n_heads)], axis=1)
    return x, ref, (0, 2 * n_heads - 1)


def q4_arms(M, K):
    return M % 16 == 0 and K % 128 == 0


def f16_arms(M, K):
    tiles, per_wg = M // 16, 8 if M > 64 else 4 if M > 32 else 2 if M > 16 else 1
    return M % 16 == 0 and K % 32 == 0 and tiles % per_wg == 0


def _arms(kind, M, K):
    return q4_arms(M, K) if kind == "q4" else f16_arms(M, K)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (1 << 32)


def _simple(name, kind, make, bars, control=True, M=None, K=None, armed=None):
    """one producer, one consumer over all of X. make(b) -> (x, ref, member range[, x_off]); M, K: how the consumer reads X"""
    b = _B(_seed(name))
    got = make(b)
    x, ref, rng_ = got[:3]
    x_off = got[3] if len(got) > 3 else 0
    M, K = M or ref.shape[0], K or ref.shape[1]
    c = b.consume(kind, x, x_off, M, K)
    armed = _arms(kind, M, K) if armed is None else armed
    tagged = None if armed == "any" else ({rng_} if armed else set())
    return Case(name, kind, b.program(), [Step(None, ref.reshape(M, K), tagged, [c])], bars, x, x_off, control=control)


# ── the table ──────────────────────────────────────────────────────────────────────────────────────────────────────────

# (M, K): smallest; two workgroups per row with a ragged second chunk; three m-tiles; the NPT = 16 split form; the looping
# NPT = 0 form (scalar piece stores); 8 m-tiles; 5 m-tiles (Q4 pads to 8, f16 refuses); widths only f16 may arm
ROW_SHAPES = [(16, 128), (16, 384), (48, 512), (32, 4096), (16, 8320), (128, 256), (80, 256), (16, 96), (16, 288), (32, 160)]
ELT_SHAPES = [(16, 128), (48, 384), (128, 8192), (16, 96)]  # (128, 8192): n = 2^20, the first length of the four-per-thread form
ATTN_SHAPES = [(64, 2, 16), (128, 3, 32), (64, 3, 16)]      # (d_head, heads, seq_q): K = 128, 384, 192 (f16 only)

_BUILDERS = {}


for _kind in ("q4", "f16"):
    for _M, _K in ROW_SHAPES:
        _BUILDERS[f"row_{_M}x{_K}_{_kind}"] = (lambda n, k=_kind, M=_M, K=_K: _simple(n, k, lambda b: _row_chain(b, M, K)[:3], BARS["rms"]))
    for _form in ("add_norm_mul", "add_norm"):
        _BUILDERS[f"row_{_form}_16x384_{_kind}"] = (lambda n, k=_kind, f=_form: _simple(n, k, lambda b: _row_chain(b, 16, 384, f)[:3], BARS["rms"]))
    for _M, _K in ELT_SHAPES:
        _BUILDERS[f"elt_{_M}x{_K}_{_kind}"] = (lambda n, k=_kind, M=_M, K=_K: _simple(n, k, lambda b: _silu_chain(b, M * K), BARS["silu"], M=M, K=K))
    # a flat hook may be re-factored: a chain of 32 * 256 elements read as 16 rows of 512
    _BUILDERS[f"elt_refactored_{_kind}"] = (lambda n, k=_kind: _simple(n, k, lambda b: _silu_chain(b, 32 * 256), BARS["silu"], M=16, K=512))
    # X at a 16-byte aligned offset keeps the four-per-thread form, at offset 1 the chain drops to the scalar one: values must hold either way
    for _off in (4, 1):
        _BUILDERS[f"elt_offset{_off}_{_kind}"] = (lambda n, k=_kind, o=_off: _simple(n, k, lambda b: _silu_chain(b, 128 * 8192, o, 3) + (o,), BARS["silu"],
                                                                                M=128, K=8192, armed="any"))
    for _dh, _nh, _sq in ATTN_SHAPES:
        _BUILDERS[f"attn_{_dh}x{_nh}_q{_sq}_{_kind}"] = (lambda n, k=_kind, d=_dh, h=_nh, s=_sq: _simple(n, k, lambda b: _attention(b, d, h, s), BARS["attn"]))


def _qkv(name, kind):
    """three matmuls over the same X right behind the chain: one launch of 3 ops, the first takes the producer's operand"""
    b = _B(_seed(name))
    x, ref, rng_, _ = _row_chain(b, 16, 256)
    cs = [b.consume(kind, x, 0, 16, 256, N) for N in (128, 64, 64)]
    return Case(name, kind, b.program(), [Step(None, ref, {rng_}, cs)], BARS["rms"], x, 0, group=(cs[0].op, cs[2].op, 3), control=True)


def _mixed(name, order):
    """a Q4 qmatmul and an f16 matmul over the same X: the first arms the producer, the second prepares its own operand"""
    b = _B(_seed(name))
    x, ref, rng_, _ = _row_chain(b, 16, 256)
    cs = [b.consume(k, x, 0, 16, 256) for k in order]
    return Case(name, "mixed", b.program(), [Step(None, ref, {rng_}, cs)], BARS["rms"], x, 0, control=True)


def _rewritten(name, kind):
    """producer, matmul, a second producer over the same X, a second matmul: each matmul is armed by its own producer. The first
    matmul's rows are gone when the buffers are read: they are norm * gain of the first chain, one f32 product per element."""
    b = _B(_seed(name))
    M, K = 16, 256
    x, _, r1, i_norm = _row_chain(b, M, K)
    nrm1, g1 = b.ops[i_norm].dst, b.ops[r1[1]].src1
    c1 = b.consume(kind, x, 0, M, K, x_of=lambda bufs: (bufs[nrm1][:M * K] * bufs[g1][:M * K]).reshape(M, K))
    s2, g2, nrm2 = b.uni(M * K), b.uni(M * K, 0.5, 1.5), b.buf(np.zeros(M * K))
    lo = b.op(DeviceOp.rmsnorm(nrm2, s2, M, K, 1e-5))
    hi = b.op(DeviceOp.elementwise("mul", x, nrm2, g2, M * K))
    c2 = b.consume(kind, x, 0, M, K)
    ref = rms64(b.vals[s2].reshape(M, K), 1e-5) * b.vals[g2].reshape(M, K).astype(f64)
    return Case(name, kind, b.program(), [Step(None, ref, {r1, (lo, hi)}, [c1, c2])], BARS["rms"], x, 0, downloads=[nrm1, g1], control=True)


def _stale_scratch(name):
    """an M = 128 matmul over rows of magnitude 1e30 leaves its pieces in the scratch; the chain then feeds an M = 80 Q4 matmul whose
    padded m-tiles 5..7 keep them: rows 0..79 right, the 48 sentinel rows behind them untouched"""
    b = _B(_seed(name))
    K = 256
    big = b.buf(b.rng.choice([-1e30, 1e30], 128 * K) * b.rng.uniform(0.5, 1.0, 128 * K))
    c0 = b.consume("q4", big, 0, 128, K)
    x, ref, rng_, _ = _row_chain(b, 80, K)
    c1 = b.consume("q4", x, 0, 80, K, tail=48 * N_OUT)
    return Case(name, "q4", b.program(), [Step(None, ref, {rng_}, [c0, c1])], BARS["rms"], x, 0, downloads=[big], control=True)


for _kind in ("q4", "f16"):
    _BUILDERS[f"group_qkv_{_kind}"] = lambda n, k=_kind: _qkv(n, k)
    _BUILDERS[f"rewritten_x_{_kind}"] = lambda n, k=_kind: _rewritten(n, k)
_BUILDERS["mixed_q4_then_f16"] = lambda n: _mixed(n, ("q4", "f16"))
_BUILDERS["mixed_f16_then_q4"] = lambda n: _mixed(n, ("f16", "q4"))
_BUILDERS["stale_scratch_q4"] = _stale_scratch


# ── near misses: the stale producer must not be armed, the values follow the reference ─────────────────────────────────

def _writer(name, kind, writer):
    """[rmsnorm -> mul] -> X, one op that rewrites rows of X, the matmul over X (M = 16, K = 128)"""
    b = _B(_seed(name))
    M, K = 16, 128
    x, ref, _, _ = _row_chain(b, M, K, x_rows=32 if writer == "wider_chain" else None)
    ref = ref.copy()
    steps_extra = []
    if writer in ("slice_assign", "slice_assign_dyn"):
        p = b.uni(K)
        row, patch = 5, K if writer == "slice_assign_dyn" else 0
        w = b.op(DeviceOp.slice_assign(x, p, K, 1, 0 if patch else row * K, row * K, 1, K, 0, 1, K, patch))
        base = ref.copy()
        ref[row] = b.vals[p]
        if patch:  # refreshed to a second position between two executions (the chain rewrites every row first)
            r2 = base.copy()
            r2[11] = b.vals[p]
            steps_extra.append((w, b.ops[w].with_(dst_offset=11 * K), r2))
    elif writer == "neg":
        b.op(DeviceOp.elementwise("neg", x, x, x, M * K))
        ref = -ref
    elif writer == "softmax":
        b.op(DeviceOp.softmax(x, x, M, K))
        ref = softmax64(ref)
    elif writer == "wider_chain":  # a second chain over 32 rows starting at X: a hook that does not fit, yet writes the rows
        s2, g2, nrm2 = b.uni(32 * K), b.uni(32 * K, 0.5, 1.5), b.buf(np.zeros(32 * K))
        b.op(DeviceOp.rmsnorm(nrm2, s2, 32, K, 1e-5))
        b.op(DeviceOp.elementwise("mul", x, nrm2, g2, 32 * K))
        ref = (rms64(b.vals[s2].reshape(32, K), 1e-5) * b.vals[g2].reshape(32, K).astype(f64))[:16]
    c = b.consume(kind, x, 0, M, K)
    steps = [Step(None, ref, set(), [c])]
    for w, new_op, r2 in steps_extra:
        ops = list(b.ops)
        ops[w] = new_op
        steps.append(Step(ops, r2, set(), [c]))
    bars = BARS["rms"] if writer != "softmax" else dict(atol=1e-6, rtol=1e-5)  # softmax of O(1) rows: values near 1 / K
    return Case(name, kind, b.program(), steps, bars, x, 0)


def _partial(name, kind, which):
    """the matmul reads part of what the producer wrote: no hook fits"""
    b = _B(_seed(name))
    if which in ("first_half", "second_half"):  # 16 of a 32-row chain
        K = 128
        x, ref, _, _ = _row_chain(b, 32, K)
        off = 0 if which == "first_half" else 16 * K
        c = b.consume(kind, x, off, 16, K)
    elif which == "strided":  # 128 columns of 256-column rows
        x, ref, _, _ = _row_chain(b, 16, 256)
        c = b.consume(kind, x, 0, 16, 128, x_rs=256)
    elif which == "m24":
        x, ref, _, _ = _row_chain(b, 24, 128)
        c = b.consume(kind, x, 0, 24, 128)
    else:  # k192: no whole 128-column steps (Q4)
        x, ref, _, _ = _row_chain(b, 16, 192)
        c = b.consume(kind, x, 0, 16, 192)
    return Case(name, kind, b.program(), [Step(None, ref, set(), [c])], BARS["rms"], x, 0)


def _refresh(name, kind, what):
    """a static refresh moves the plan: the tag and the values follow"""
    b = _B(_seed(name))
    M, K = 16, 128
    x, ref, rng_, i_norm = _row_chain(b, M, K, x_rows=32)
    c = b.consume(kind, x, 0, M, K)
    steps = [Step(None, ref, {rng_}, [c])]
    if what == "input_offset":  # to the uploaded rows 16..31 and back
        far = b.ops[c.op].with_(input_offset=M * K) if kind == "q4" else b.ops[c.op].with_(geom=replace(b.ops[c.op].geom, a_offset=M * K))
        ops = list(b.ops)
        ops[c.op] = far
        steps.append(Step(ops, ref, set(), [replace(c, x_off=M * K)]))
        steps.append(Step(list(b.ops), ref, {rng_}, [c]))
    else:  # the producer's eps
        ops = list(b.ops)
        ops[i_norm] = ops[i_norm].with_(eps=1e-2)
        s = b.vals[b.ops[i_norm].src].reshape(M, K)
        g = b.vals[b.ops[rng_[1]].src1].reshape(M, K).astype(f64)
        steps.append(Step(ops, rms64(s, 1e-2) * g, {rng_}, [c]))
    return Case(name, kind, b.program(), steps, BARS["rms"], x, 0)


for _kind in ("q4", "f16"):
    for _w in ("slice_assign", "neg", "softmax", "slice_assign_dyn", "wider_chain"):
        _BUILDERS[f"writer_{_w}_{_kind}"] = lambda n, k=_kind, w=_w: _writer(n, k, w)
    for _p in ("first_half", "second_half", "strided", "m24"):
        _BUILDERS[f"partial_{_p}_{_kind}"] = lambda n, k=_kind, p=_p: _partial(n, k, p)
    for _r in ("input_offset", "eps"):
        _BUILDERS[f"refresh_{_r}_{_kind}"] = lambda n, k=_kind, r=_r: _refresh(n, k, r)
_BUILDERS["partial_k192_q4"] = lambda n: _partial(n, "q4", "k192")

CASE_NAMES = list(_BUILDERS)
CONTROL_NAMES = [n for n in CASE_NAMES if n.startswith(("row_", "elt_", "attn_", "group_", "mixed_", "rewritten_", "stale_"))]
_cache = {}


def build_case(name) -> Case:
    """built once per process and shared: nothing may modify a case"""
    if name not in _cache:
        _cache[name] = _BUILDERS[name](name)
    return _cache[name]


def matmul_only(case: Case, step: Step, bufs: dict) -> DeviceProgram:
    """the step's matmuls alone, over the rows the device produced (uploaded): they prepare their own A operand. A consumer
    whose rows were overwritten later reads them from a buffer of its own."""
    ops_all = case.prog.ops if step.ops is None else step.ops
    sizes, ups, ops = list(case.prog.buffer_sizes), [], []
    weights = {c.weight[0] for c in step.consumers if c.kind == "f16"}
    for io in case.prog.initial_uploads:
        if io.buf_idx in weights or io.buf_idx in {c.y_buf for c in step.consumers}:
            ups.append(io)
    xs = {}
    for c in step.consumers:
        op = ops_all[c.op]
        if c.x_of:
            sizes.append(c.M * c.K)
            ups.append(ProgramIO(len(sizes) - 1, np.ascontiguousarray(c.x(bufs), f32).ravel()))
            op = op.with_(input=len(sizes) - 1) if c.kind == "q4" else op.with_(a=len(sizes) - 1)
        else:
            xs[c.x_buf] = bufs[c.x_buf]
        ops.append(op)
    ups += [ProgramIO(b, np.ascontiguousarray(v, f32)) for b, v in xs.items()]
    return DeviceProgram(ops=ops, buffer_sizes=sizes, initial_uploads=ups, qweights=list(case.prog.qweights))
