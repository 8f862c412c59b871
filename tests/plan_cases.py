"""Seeded random DeviceOps and DevicePrograms for the schedule / planner tests (tests/test_schedule.py): one generator per op
kind the dependency schedule models (zgml_amd/csrc/schedule.hip op_access), each drawing offsets and strides that keep every
access inside buffers of `size` f32 elements, and random programs over a few small buffers with deliberate partial overlaps,
in-place ops and barriers."""
import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, FusedEwStep, MatMulGeometry, ProgramIO, QuantizedWeightUpload

f32 = np.float32
UNARY = ("neg", "abs", "relu", "sgn", "step")
BINARY = ("add", "mul")
KINDS = ("elementwise", "fused_elementwise", "matmul", "qmatmul", "softmax", "layernorm", "rmsnorm", "reduce", "repeat",
         "slice_assign", "slice_assign_dyn", "rope", "attention", "attention_mask", "kvq_store", "attention_kvq")
# kinds a random program is made of (qmatmul and the quantised-KV ops need weights / cache layouts of their own)
PROGRAM_KINDS = ("elementwise", "elementwise", "elementwise", "fused_elementwise", "matmul", "softmax", "layernorm", "rmsnorm",
                 "reduce", "repeat", "slice_assign", "rope", "attention", "attention_mask")


def _ri(rng, lo, hi):
    """uniform integer in [lo, hi]"""
    return int(rng.integers(lo, hi + 1))


def _off(rng, size, extent):
    return _ri(rng, 0, max(0, size - extent))


def random_op(rng, kind, n_bufs, size):
    """One op of `kind` over buffers 0..n_bufs-1 of `size` elements. Returns (op, seq_kv_bound or 0). Buffers are drawn
    independently, so sources and destinations may be the same buffer at overlapping offsets."""
    b = lambda: _ri(rng, 0, n_bufs - 1)  # noqa: E731
    if kind == "elementwise":
        n = _ri(rng, 1, min(16, size))
        op = str(rng.choice(UNARY + BINARY + BINARY))
        return DeviceOp.elementwise(op, b(), b(), b(), n, _off(rng, size, n), _off(rng, size, n), _off(rng, size, n)), 0
    if kind == "fused_elementwise":
        n = _ri(rng, 1, min(12, size))
        steps = []
        for _ in range(_ri(rng, 1, 3)):
            op = str(rng.choice(UNARY + BINARY))
            steps.append(FusedEwStep(op, bool(rng.integers(2)), b(), _off(rng, size, n)) if op in BINARY else FusedEwStep(op))
        return DeviceOp.fused_elementwise(steps, n, b(), b(), _off(rng, size, n), _off(rng, size, n)), 0
    if kind == "matmul":
        M, N, K = _ri(rng, 1, 3), _ri(rng, 1, 3), _ri(rng, 1, 3)
        acs, bcs = _ri(rng, 1, 2), _ri(rng, 1, 2)
        ars, brs, drs = _ri(rng, K * acs, K * acs + 2), _ri(rng, N * bcs, N * bcs + 2), _ri(rng, N, N + 2)
        ea, eb, ed = (M - 1) * ars + (K - 1) * acs + 1, (K - 1) * brs + (N - 1) * bcs + 1, (M - 1) * drs + N
        g = MatMulGeometry(M, N, K, ars, acs, brs, bcs, _off(rng, size, ea), _off(rng, size, eb), _off(rng, size, ed), drs)
        return DeviceOp.matmul(b(), b(), b(), g), 0
    if kind == "qmatmul":  # weight 0: K x N (qmatmul_weight)
        M, K, N = _ri(rng, 1, 3), 4, 4
        irs, drs = _ri(rng, K, K + 3), _ri(rng, N, N + 3)
        ei, ed = (M - 1) * irs + K, (M - 1) * drs + N
        return DeviceOp.qmatmul(b(), b(), 0, M, N, K, _off(rng, size, ei), irs, _off(rng, size, ed), drs), 0
    if kind in ("softmax", "layernorm", "rmsnorm"):
        rows, cols = _ri(rng, 1, 3), _ri(rng, 1, 8)
        n = rows * cols
        return getattr(DeviceOp, kind)(b(), b(), rows, cols, **({} if kind == "softmax" else {"eps": 1e-5}),
                                       src_offset=_off(rng, size, n), dst_offset=_off(rng, size, n)), 0
    if kind == "reduce":
        n_out, rs = _ri(rng, 1, 4), _ri(rng, 1, 5)
        return DeviceOp.reduce(str(rng.choice(("sum", "max"))), b(), b(), n_out, rs, _off(rng, size, n_out * rs),
                               _off(rng, size, n_out)), 0
    if kind == "repeat":
        w, r = _ri(rng, 1, 4), _ri(rng, 1, 3)
        if rng.integers(2):  # dense source: a tile copy
            src_strides, ext = (1, w, w, w), w
        else:  # a strided source: the generic index math
            src_strides, ext = (2, 2 * w, 2 * w, 2 * w), 2 * w - 1
        n = w * r
        return DeviceOp.repeat(b(), b(), n, (w, 1, 1, 1), (w, r, 1, 1), src_strides, (1, w, n, n), _off(rng, size, ext),
                               _off(rng, size, n)), 0
    if kind in ("slice_assign", "slice_assign_dyn"):
        rows, cols = _ri(rng, 1, 4), _ri(rng, 1, 3)
        srs, scs = (1, _ri(rng, rows, rows + 2)) if rng.integers(2) else (_ri(rng, cols, cols + 2), 1)
        drs, dcs = (1, _ri(rng, rows, rows + 2)) if rng.integers(2) else (_ri(rng, cols, cols + 2), 1)
        es, ed = (rows - 1) * srs + (cols - 1) * scs + 1, (rows - 1) * drs + (cols - 1) * dcs + 1
        if kind == "slice_assign":
            do = _off(rng, size, ed)
            return DeviceOp.slice_assign(b(), b(), rows, cols, do, do, drs, dcs, _off(rng, size, es), srs, scs, 0), 0
        patch = _ri(rng, 1, 3)
        base = _off(rng, size, ed + 2 * patch)
        pos = _ri(rng, 0, 2)
        return DeviceOp.slice_assign(b(), b(), rows, cols, base, base + pos * patch, drs, dcs, _off(rng, size, es), srs, scs, patch), 0
    if kind == "rope":
        hd, seq = _ri(rng, 1, 3), _ri(rng, 1, 3)
        d = 2 * hd
        src_cs, cs_cs = _ri(rng, d, d + 3), _ri(rng, d, d + 3)
        es, ec, ed = (seq - 1) * src_cs + d, (seq - 1) * cs_cs + d, seq * d
        return DeviceOp.rope(b(), b(), b(), hd, seq, _off(rng, size, es), _off(rng, size, ec), _off(rng, size, ed), 1, src_cs, cs_cs), 0
    if kind in ("attention", "attention_mask"):
        dh, sq, skv = _ri(rng, 1, 4), _ri(rng, 1, 2), _ri(rng, 1, 4)
        bound = skv + _ri(rng, 0, 2)
        qcs, kcs, vcs, dcs = (_ri(rng, dh, dh + 2) for _ in range(4))
        mrs, mcs = 1, _ri(rng, bound, bound + 2)
        eq, ek, ev, ed = (sq - 1) * qcs + dh, (bound - 1) * kcs + dh, (bound - 1) * vcs + dh, (sq - 1) * dcs + dh
        em = (sq - 1) * mcs + bound
        has = kind == "attention_mask"
        return DeviceOp.attention(b(), b(), b(), b(), b(), has, dh, sq, skv, 0.5, _off(rng, size, eq), _off(rng, size, ek),
                                  _off(rng, size, ev), _off(rng, size, em), _off(rng, size, ed), 1, qcs, 1, kcs, 1, vcs, mrs,
                                  mcs, 1, dcs), bound
    if kind == "kvq_store":
        n_cols = _ri(rng, 2, 3)
        col = _ri(rng, 0, n_cols - 1)
        return DeviceOp.kvq_store(b(), b(), 32, 32, n_cols, _off(rng, size, 32), 0, col, 0), 0
    if kind == "attention_kvq":
        n_cols, sq = _ri(rng, 2, 3), _ri(rng, 1, 2)
        skv = _ri(rng, 1, n_cols)
        k = b()
        v = (k + 1) % n_bufs
        qcs, dcs = _ri(rng, 32, 34), _ri(rng, 32, 34)
        mcs = _ri(rng, n_cols, n_cols + 2)
        eq, ed, em = (sq - 1) * qcs + 32, (sq - 1) * dcs + 32, (sq - 1) * mcs + n_cols
        return DeviceOp.attention_kvq(b(), b(), k, v, b(), bool(rng.integers(2)), 32, sq, skv, 0.25, 32, n_cols, 0, 0,
                                      _off(rng, size, eq), qcs, _off(rng, size, ed), dcs, _off(rng, size, em), 1, mcs), n_cols
    raise ValueError(kind)


def qmatmul_weight(rng, K=4, N=4):
    return QuantizedWeightUpload(rng.integers(-8, 8, K * N).astype(np.int8), (rng.random(K * N // 4) * 0.1 + 0.01).astype(f32), K, N, 4)


def random_values(rng, n):
    """O(1) f32 values (read as int8 bytes and scales where a quantised-KV cache lies: finite either way)"""
    return rng.uniform(-1.5, 1.5, n).astype(f32)


def random_program(seed, n_ops=None):
    """8-40 ops over 3-6 buffers of 48 elements (offsets drawn independently: partial overlaps and in-place forms are common),
    0-2 barriers. Returns (ops, buffer_sizes, barriers, seq_kv_bound)."""
    rng = np.random.default_rng(seed)
    n_bufs, size = _ri(rng, 3, 6), 48
    n_ops = n_ops or _ri(rng, 8, 40)
    ops, bounds = [], []
    for _ in range(n_ops):
        op, bound = random_op(rng, str(rng.choice(PROGRAM_KINDS)), n_bufs, size)
        ops.append(op)
        bounds.append(bound)
    barriers = sorted({_ri(rng, 1, n_ops - 1) for _ in range(_ri(rng, 0, 2))})
    return ops, [size] * n_bufs, barriers, bounds


def program_with_inputs(ops, sizes, rng, qweights=()):
    """`ops` over buffers filled with random values (every buffer uploaded)"""
    ups = [ProgramIO(i, random_values(rng, s)) for i, s in enumerate(sizes)]
    return DeviceProgram(ops=list(ops), buffer_sizes=list(sizes), initial_uploads=ups, qweights=list(qweights))


# ── programs the HIP planner fuses (tests/test_hip_plan_legality.py, tests/test_hip_plan_random.py) ─────────────────────

def decode_group(dh=64, n_heads=2, pos=3, max_seq=8, has_mask=True, base=0):
    """One kv group of a decode step as the LLaMA lowering emits it, over buffers base..base+8: per head rope q -> attention
    -> row store, rope k -> K store, V store (the stores at column `pos`, patch_stride = d_head). Returns (ops, sizes) with
    the buffers P projections, CS cos|sin row, QR, KR, KC, VC, MASK, AO, O at base + 0..8."""
    P, CS, QR, KR, KC, VC, MASK, AO, O = range(base, base + 9)
    hd = dh // 2
    ops = [DeviceOp.rope(QR, P, CS, hd, 1, h * dh, 0, h * dh, 1, dh, dh) for h in range(n_heads)]
    ops += [DeviceOp.rope(KR, P, CS, hd, 1, n_heads * dh, 0, 0, 1, dh, dh),
            DeviceOp.slice_assign(KC, KR, dh, 1, 0, pos * dh, 1, dh, 0, 1, dh, dh),
            DeviceOp.slice_assign(VC, P, dh, 1, 0, pos * dh, 1, dh, (n_heads + 1) * dh, 1, dh, dh)]
    for h in range(n_heads):
        ops.append(DeviceOp.attention(AO, QR, KC, VC, MASK, has_mask, dh, 1, pos + 1, dh ** -0.5, h * dh, 0, 0, 0, h * dh,
                                      1, dh, 1, dh, 1, dh, 1, max_seq, 1, dh))
        ops.append(DeviceOp.slice_assign(O, AO, dh, 1, h * dh, h * dh, 1, dh, h * dh, 1, dh, 0))
    sizes = [(n_heads + 2) * dh, dh, n_heads * dh, dh, max_seq * dh, max_seq * dh, max_seq, n_heads * dh + 4, n_heads * dh + 4]
    return ops, sizes


def group_uploads(rng, sizes, pos, base=0):
    """O(1) values everywhere; the mask row open up to `pos`, closed after it; cos|sin a real rotation"""
    ups = [ProgramIO(base + b, rng.uniform(-1, 1, s).astype(f32)) for b, s in enumerate(sizes)]
    dh = sizes[1]
    ang = rng.uniform(0, 3, dh // 2)
    ups[1] = ProgramIO(base + 1, np.concatenate([np.cos(ang), np.sin(ang)]).astype(f32))
    ups[6] = ProgramIO(base + 6, np.where(np.arange(sizes[6]) <= pos, 0, -np.inf).astype(f32))
    return ups


def random_fusable_program(seed):
    """A random program of the patterns the planner fuses, over shared vector buffers with aliasing injected on purpose:
    M = 1 mat-vecs (N % 32 == 0) with mul / rmsnorm producers and add / mul consumers, [add ->] rmsnorm [-> mul] rows,
    elementwise chains, rope -> slice_assign, and one decode-attention group. Operands and destinations are drawn from the
    same few buffers at offsets that are multiples of 4 (so the passes' alignment rules hold) and may meet at shifted
    indices. Returns a DeviceProgram with every buffer uploaded; values stay O(1)."""
    rng = np.random.default_rng(seed)
    K, S, n_vec = 256, 320, 6
    rows, cols = 4, 64
    sizes = [S] * n_vec + [rows * cols + cols] * 2
    ops, qweights = [], []

    def self_ok(o):
        """an op whose store meets its own inputs at another index races inside its own kernel, fused or not: the aliasing
        injected here is BETWEEN ops (in-place at the same index is fine for the elementwise and row ops)"""
        f = o.f
        if o.kind == "elementwise":
            pairs = [(f["src0"], f["src0_offset"]), (f["src1"], f["src1_offset"])]
            n = f["n"]
            return all(b != f["dst"] or bo == f["dst_offset"] or bo + n <= f["dst_offset"] or f["dst_offset"] + n <= bo for b, bo in pairs)
        if o.kind == "rmsnorm":
            n = f["rows"] * f["cols"]
            so, do = f["src_offset"], f["dst_offset"]
            return f["src"] != f["dst"] or so == do or so + n <= do or do + n <= so
        if o.kind == "qmatmul":
            return f["input"] != f["dst"] or f["input_offset"] + f["K"] <= f["dst_offset"] or f["dst_offset"] + f["N"] <= f["input_offset"]
        if o.kind == "rope":
            n = 2 * f["half_d"] * f["seq_len"]
            return all(b != f["dst"] or bo + n <= f["dst_off"] or f["dst_off"] + n <= bo for b, bo in ((f["src"], f["src_off"]), (f["cos_sin"], f["cs_off"])))
        if o.kind == "slice_assign":
            n = f["rows"] * f["cols"]
            return f["src"] != f["dst"] or f["src_offset"] + n <= f["dst_offset"] or f["dst_offset"] + n <= f["src_offset"]
        return True

    def add(o):
        if self_ok(o):
            ops.append(o)
            return True
        return False
    vec = lambda: _ri(rng, 0, n_vec - 1)                    # noqa: E731
    off = lambda n: 4 * _ri(rng, 0, (S - n) // 4)           # noqa: E731
    same_or_shift = lambda: 0 if rng.random() < 0.6 else 4 * _ri(rng, 1, 8)  # noqa: E731
    for _ in range(_ri(rng, 3, 7)):
        pat = _ri(rng, 0, 3)
        if pat == 0:  # [rmsnorm ->] mul -> mat-vec -> consumers
            a, g, x = (int(v) for v in rng.permutation(n_vec)[:3]) if rng.random() < 0.5 else (vec(), vec(), vec())
            ao, go, xo = off(K), off(K), off(K)
            if rng.random() < 0.5:
                n_buf = int(rng.choice([v for v in range(n_vec) if v not in (a, g, x)]))
                n_off = off(K)
                if add(DeviceOp.rmsnorm(n_buf, a, 1, K, 1e-5, src_offset=ao, dst_offset=n_off)):
                    a, ao = n_buf, n_off
            if not add(DeviceOp.elementwise("mul", x, a, g, K, xo, ao, go)):
                continue
            for _ in range(_ri(rng, 1, 2)):  # one or two consumers (q / k / v style)
                y, yo = vec(), off(K)
                qweights.append(QuantizedWeightUpload(rng.integers(-8, 8, K * K).astype(np.int8),
                                                      (rng.random(K * K // 32) * 0.01 + 0.002).astype(f32), K, K, 32))
                if not add(DeviceOp.qmatmul(y, x, len(qweights) - 1, 1, K, K, input_offset=xo, dst_offset=yo)):
                    continue
                cur, co = y, yo
                for _ in range(_ri(rng, 0, 2)):
                    d, r = vec(), vec()
                    do, ro = (co + same_or_shift()) % (S - K + 4) // 4 * 4, off(K)
                    if not add(DeviceOp.elementwise(str(rng.choice(BINARY)), d, cur, r, K, do, co, ro)):
                        break
                    cur, co = d, do
        elif pat == 1:  # [add ->] rmsnorm [-> mul] rows
            R0, R1 = n_vec, n_vec + 1
            h = int(rng.choice([R0, R1]))
            hs = cols * _ri(rng, 0, 1)
            if not add(DeviceOp.elementwise("add", h, R0, R1, rows * cols, hs, 0, cols * _ri(rng, 0, 1))):
                continue
            nb = int(rng.choice([R0, R1]))
            ns = cols * _ri(rng, 0, 1)
            if add(DeviceOp.rmsnorm(nb, h, rows, cols, 1e-5, src_offset=hs, dst_offset=ns)) and rng.random() < 0.7:
                add(DeviceOp.elementwise("mul", int(rng.choice([R0, R1])), nb, int(rng.choice([R0, R1])), rows * cols,
                                                cols * _ri(rng, 0, 1), ns, cols * _ri(rng, 0, 1)))
        elif pat == 2:  # an elementwise chain
            n = 4 * _ri(rng, 8, 64)
            cur, co = vec(), off(n)
            for _ in range(_ri(rng, 2, 4)):
                d, r = vec(), vec()
                do = min(S - n, co + same_or_shift()) // 4 * 4 if rng.random() < 0.5 else off(n)
                op = str(rng.choice(BINARY + ("neg", "abs")))
                if not add(DeviceOp.elementwise(op, d, cur, r, n, do, co, off(n))):
                    break
                cur, co = d, do
        else:  # rope -> slice_assign of its rows
            hd, seq = 8, 2
            src, cs, dst, sl = vec(), vec(), vec(), vec()
            ro = off(seq * 2 * hd)
            if not add(DeviceOp.rope(dst, src, cs, hd, seq, off(2 * hd * seq), off(2 * hd * seq), ro, 1, 2 * hd, 2 * hd)):
                continue
            so = off(2 * hd * seq)
            add(DeviceOp.slice_assign(sl, dst, 2 * hd, seq, so, so, 1, 2 * hd, ro, 1, 2 * hd, 0))
    # one decode-attention group over buffers of its own; sometimes its row stores land in a shared vector buffer
    pos = _ri(rng, 0, 6)
    g_ops, g_sizes = decode_group(pos=pos, base=len(sizes))
    if rng.random() < 0.3:
        v = vec()
        g_ops = [o.with_(dst=v, dst_base_offset=o.dst_base_offset + 4 * (v + 1), dst_offset=o.dst_offset + 4 * (v + 1))
                 if o.kind == "slice_assign" and o.patch_stride == 0 else o for o in g_ops]
    ups = [ProgramIO(b, rng.uniform(-1, 1, s).astype(f32)) for b, s in enumerate(sizes)]
    ups += group_uploads(rng, g_sizes, pos, base=len(sizes))
    sizes += g_sizes
    return DeviceProgram(ops=ops + g_ops, buffer_sizes=sizes, initial_uploads=ups, qweights=qweights)
