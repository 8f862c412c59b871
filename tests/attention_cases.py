"""Named attention cases for every kernel route of the batched attention launch (zgml_amd/csrc/kernels_generic.hip
launch_attention_batch: generic, dense, rows, tiles), the fused decode form and the stand-alone quantised-KV kernel, plus the
skip-rule variants of a few of them (tests/test_attention_cases_host.py pins the expected side on the CPU,
tests/test_hip_attention_routes.py runs the device).

A case is a DeviceProgram whose heads each own their buffers (q, k, v, mask, dst), so the heads of a case are independent
and share one launch. Inputs are standard_normal f32, scale = d_head ** -0.5; every destination is uploaded as -7 sentinels so
gaps a destination stride leaves can be checked. Masks are causal (query qi sees keys 0 .. seq_kv - seq_q + qi) plus a few DEAD
columns that no query sees.

The skip rule (src/backend/reference.zig:612, :631; oracle/zgml_oracle.c zo_attention): a key whose mask is non-finite, or whose
score comes out non-finite, is skipped BEFORE its V row is read. The variants put non-finite values only where the reference
skips for every query:
  masked   K rows of the dead columns are NaN, their V rows a NaN / +inf / -inf mix (kvq: the block scales instead)
  inf_k    one dead column is unmasked, its K row is +inf (the score is non-finite: dropped) and its V row is poisoned
  nan_q    query column 1 is all NaN: its output is exactly zero, every other query is untouched
A live key is never poisoned (a live key whose weight underflows to 0 makes the reference itself return NaN)."""
from dataclasses import dataclass, field

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO
from tests.plan_cases import decode_group, group_uploads

f32 = np.float32
SENTINEL = f32(-7)
VARIANTS = ("masked", "inf_k", "nan_q")
NAN_QUERY = 1
KVQ_KIND = 14  # ZGML_DOP_ATTENTION_KVQ: its launches carry no tag, the plan text shows the kind


@dataclass
class Case:
    name: str
    prog: DeviceProgram
    tag: str                      # what the plan text must carry for the attention launch
    outs: list                    # destination buffers
    dead: list = field(default_factory=list)      # per attention op: the columns no query sees
    refresh: tuple = ()           # further seq_kv values run on the same compiled program
    twice: bool = False           # 2048-key cases: a second execute gives identical bits
    inf_col: int = -2             # index into `dead` of the column the inf_k variant opens
    # cases whose query is computed inside the program: where the nan_q variant puts its NaNs (buffer, indices) and which
    # elements of each output buffer it zeroes {buffer: indices}; otherwise query NAN_QUERY of every attention op
    nan_q_in: tuple = None
    nan_q_zero: dict = None

    def attention_ops(self):
        return [o for o in self.prog.ops if o.kind in ("attention", "attention_kvq")]


def dead_columns(skv):
    return sorted({3, 7, skv // 2, skv - 1}) if skv >= 16 else []  # (key 0 stays live: seq_kv refreshed to 1 keeps a key)


def causal_mask(sq, skv, dead=(), closed=None):
    """[sq, skv] additive mask; closed = {qi: first n keys shut}"""
    m = np.zeros((sq, skv), f32)
    for qi in range(sq):
        m[qi, max(1, skv - sq + qi + 1):] = -np.inf
    m[:, list(dead)] = -np.inf
    for qi, n in (closed or {}).items():
        m[qi, :n] = -np.inf
    return m


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.sizes, self.ups, self.ops, self.outs, self.dead = [], [], [], [], []

    def head(self, dh, sq, skv, q_rs=1, q_cs=None, k_rs=1, k_cs=None, v_rs=1, v_cs=None, mask_rs=1, mask_cs=None, dst_rs=1,
             dst_cs=None, q_off=0, has_mask=True, closed=None):
        q_cs, k_cs, v_cs = (dh if c is None else c for c in (q_cs, k_cs, v_cs))
        dst_cs = dh if dst_cs is None else dst_cs
        mask_cs = skv if mask_cs is None else mask_cs
        ext = lambda n, cs, rs: (n - 1) * cs + (dh - 1) * rs + 1  # noqa: E731
        dead = dead_columns(skv) if has_mask else []
        mask = causal_mask(sq, skv, dead, closed)
        if mask_cs == 0:  # one row for every query: the dead columns only
            mask[:] = 0
            mask[:, dead] = -np.inf
        mbuf = np.zeros((sq - 1) * mask_cs + (skv - 1) * mask_rs + 1, f32)
        for qi in range(sq):
            mbuf[qi * mask_cs + np.arange(skv) * mask_rs] = mask[qi]
        base = len(self.sizes)
        Q, K, V, M, D = range(base, base + 5)
        n_q, n_k, n_v, n_d = q_off + ext(sq, q_cs, q_rs), ext(skv, k_cs, k_rs), ext(skv, v_cs, v_rs), ext(sq, dst_cs, dst_rs) + 2
        self.sizes += [n_q, n_k, n_v, mbuf.size, n_d]
        self.ups += [ProgramIO(Q, self.rng.standard_normal(n_q).astype(f32)), ProgramIO(K, self.rng.standard_normal(n_k).astype(f32)),
                     ProgramIO(V, self.rng.standard_normal(n_v).astype(f32)), ProgramIO(M, mbuf), ProgramIO(D, np.full(n_d, SENTINEL, f32))]
        self.ops.append(DeviceOp.attention(D, Q, K, V, M, has_mask, dh, sq, skv, float(dh ** -0.5), q_off, 0, 0, 0, 0, q_rs, q_cs, k_rs, k_cs,
                                           v_rs, v_cs, mask_rs, mask_cs, dst_rs, dst_cs))
        self.outs.append(D)
        self.dead.append(dead)
        return self

    def case(self, name, tag, **kw):
        return Case(name, DeviceProgram(ops=self.ops, buffer_sizes=self.sizes, initial_uploads=self.ups), tag, self.outs, self.dead, **kw)


GENERIC, DENSE, ROWS, TILES = "attention-generic", "attention-dense", "attention-rows", "attention-tiles"


def _specs():
    """name -> (tag, builder steps, Case keywords)"""
    H = lambda *a, **k: (a, k)  # noqa: E731
    return {
        # the fully strided kernel: 256 keys per tile
        "generic_dh80_three_key_blocks": (GENERIC, [H(80, 2, 600)], {}),                          # G = 3 key groups, 16 idle threads, last tile ragged
        "generic_dh320_row_pairs": (GENERIC, [H(320, 2, 300)], {}),                           # second row only for r0 < 64
        "generic_dh512_max": (GENERIC, [H(512, 2, 257)], {}),
        "generic_smallest": (GENERIC, [H(1, 1, 1, has_mask=False)], {}),
        "generic_kv_transposed": (GENERIC, [H(64, 3, 300, k_rs=300, k_cs=1, v_rs=300, v_cs=1)], {}),
        "generic_q_strided_dst_transposed": (GENERIC, [H(64, 3, 70, q_rs=4, q_cs=1, dst_rs=3, dst_cs=1)], {}),
        "generic_q_misaligned": (GENERIC, [H(64, 2, 70, q_off=3)], {}),
        "generic_k_cs_66": (GENERIC, [H(64, 2, 70, k_cs=66)], {}),
        "generic_mask_transposed": (GENERIC, [H(24, 3, 70, mask_rs=3, mask_cs=1)], {}),
        "generic_mask_shared_row": (GENERIC, [H(96, 2, 270, mask_cs=0)], {}),
        "generic_level_of_three": (GENERIC, [H(64, 2, 70), H(64, 2, 70, k_cs=66), H(64, 2, 70)], {}),  # one non-dense head takes the level
        # float4-per-lane kernel with a score buffer: 2048 keys per tile
        "dense_dh4_two_tiles": (DENSE, [H(4, 2, 2050)], {"twice": True, "refresh": (1, 2048, 2049)}),
        "dense_dh64_dh128_first_tile_shut": (DENSE, [H(64, 2, 2100, closed={1: 2048}), H(128, 2, 2100, closed={1: 2048})], {"twice": True}),
        "dense_dh8_dh256": (DENSE, [H(8, 2, 70), H(256, 2, 70)], {}),
        # streaming kernel
        "rows_dh8_loop": (ROWS, [H(8, 2, 2100)], {"twice": True, "refresh": (1,)}),         # LPK = 2: step_keys 2048 at 16 waves
        "rows_dh16": (ROWS, [H(16, 2, 1100)], {"refresh": (1,)}),
        "rows_dh256_key_per_wave": (ROWS, [H(256, 2, 200)], {"refresh": (1,)}),             # LPK = 64: four rounds, the last ragged
        "rows_dh16_4wave_blocks": (ROWS, [H(16, 15, 300)] * 18, {}),                         # 270 workgroups
        # matrix-core kernel: carriers of the skip variants
        "tiles_dh64_sq33": (TILES, [H(64, 33, 90)], {}),
        "tiles_dh128_sq16": (TILES, [H(128, 16, 37)], {}),
    }


CASE_NAMES = tuple(_specs()) + ("decode_group", "kvq_dh64")
# one representative per route for the skip variants (both V-accumulation branches of the generic kernel)
SKIP_CASES = ("generic_dh80_three_key_blocks", "generic_dh320_row_pairs", "dense_dh64_dh128_first_tile_shut", "rows_dh16", "tiles_dh64_sq33",
              "tiles_dh128_sq16", "decode_group", "kvq_dh64")
# what the cases above become when a switch takes their kernel away (switches are latched per process)
ROWS_OFF = {"rows_dh8_loop": DENSE, "rows_dh16": DENSE, "rows_dh256_key_per_wave": DENSE, "rows_dh16_4wave_blocks": DENSE,
            "tiles_dh64_sq33": DENSE, "tiles_dh128_sq16": DENSE}
TILES_OFF = {"tiles_dh64_sq33": ROWS, "tiles_dh128_sq16": ROWS}


def _decode_case():
    """plan_cases.decode_group at position 40 of a 48-column cache: two heads share the caches and one mask row; columns 0, 3, 20
    are shut. Head 0's query is rope(its slice of the projections) and its output row is stored once more, so the nan_q
    variant's places are read off the ops: the rope that feeds head 0's q, the slice_assign that copies head 0's rows."""
    pos, max_seq = 40, 48
    ops, sizes = decode_group(dh=64, n_heads=2, pos=pos, max_seq=max_seq)
    ups = group_uploads(np.random.default_rng(0xDEC0), sizes, pos)
    att = [o for o in ops if o.kind == "attention"]
    a = att[0].f
    assert all(o.f["mask"] == a["mask"] and o.f["seq_q"] == 1 for o in att)
    dead = [0, 3, 20]
    next(u.host for u in ups if u.buf_idx == a["mask"])[a["mask_off"] + np.array(dead) * a["mask_rs"]] = -np.inf
    r = np.arange(a["d_head"])
    rope = next(o.f for o in ops if o.kind == "rope" and (o.f["dst"], o.f["dst_off"]) == (a["q"], a["q_off"]))
    copy = next(o.f for o in ops if o.kind == "slice_assign" and (o.f["src"], o.f["src_offset"]) == (a["dst"], a["dst_off"]))
    assert copy["rows"] == a["d_head"] and copy["cols"] == 1
    zero = {a["dst"]: a["dst_off"] + r * a["dst_rs"], copy["dst"]: copy["dst_offset"] + r * copy["dst_row_stride"]}
    outs = sorted(zero)
    return Case("decode_group", DeviceProgram(ops, sizes, ups), "decode-attention", outs, [dead] * len(att),
                nan_q_in=(rope["src"], rope["src_off"] + r * rope["src_rs"]), nan_q_zero=zero)


def _kvq_case():
    """stand-alone attention_kvq over caches uploaded as bytes: int8 rows, then the f32 block scales.

    The quantised reference (src/quant.zig:925-1091 attentionQuantized, oracle/zgml_oracle.c zo_attention_kvq) walks flash tiles of
    8 columns and skips less than the f32 one: a masked column inside a tile that has a live one gets weight exp(-inf) = 0 TIMES its
    V scale, and a non-finite score inside a tile poisons the tile maximum. It skips, before any V read, a tile whose 8 columns are
    all masked, and a masked or non-finite-score column of the one-by-one tail (columns 32..36 here). So the dead columns are one
    whole tile (8..15) and a tail column (33), and inf_k opens the tail column."""
    rng = np.random.default_rng(0x6B76)
    dh, bs, n_cols, start, sq, skv = 64, 32, 48, 5, 3, 37
    bpc = dh // bs

    def cache():
        data = rng.integers(-127, 128, n_cols * dh).astype(np.int8)
        scales = rng.uniform(0.004, 0.02, n_cols * bpc).astype(f32)
        return np.concatenate([data.view(f32), scales])
    dead = list(range(8, 16)) + [33]
    q = rng.standard_normal(sq * dh).astype(f32)
    op = DeviceOp.attention_kvq(5, 4, 0, 1, 6, True, dh, sq, skv, float(dh ** -0.5), bs, n_cols, start, start, 0, dh, 0, dh, 0, 1, skv)
    ce = n_cols * dh // 4 + n_cols * bpc
    ups = [ProgramIO(0, cache()), ProgramIO(1, cache()), ProgramIO(4, q), ProgramIO(5, np.full(sq * dh + 2, SENTINEL, f32)),
           ProgramIO(6, causal_mask(sq, skv, dead).ravel())]
    return Case("kvq_dh64", DeviceProgram(ops=[op], buffer_sizes=[ce, ce, 1, 1, sq * dh, sq * dh + 2, sq * skv], initial_uploads=ups),
                f"kind {KVQ_KIND} ", [5], [dead], inf_col=-1)


def build_case(name, variant=None):
    if name == "decode_group":
        c = _decode_case()
    elif name == "kvq_dh64":
        c = _kvq_case()
    else:
        tag, heads, kw = _specs()[name]
        b = _Builder(sum(name.encode()) * 7919)
        for a, k in heads:
            b.head(*a, **k)
        c = b.case(name, tag, **kw)
    if variant:
        _poison(c, variant)
    return c


# ── the variants ────────────────────────────────────────────────────────────────────────────────────────────────────────────

def _host(prog, buf):
    return next(u.host for u in prog.initial_uploads if u.buf_idx == buf)


POISON_V = np.array([np.nan, np.inf, -np.inf], f32)


def _poison(c, variant):
    """in place, on the uploads of c.prog (build_case made them for this call alone)"""
    assert variant in VARIANTS
    for op, dead in zip(c.attention_ops(), c.dead):
        o = op.f
        dh, sq, skv = o["d_head"], o["seq_q"], o["seq_kv"]
        assert dead and (sq > NAN_QUERY or c.nan_q_in), c.name
        r = np.arange(dh)
        if variant == "nan_q":
            if c.nan_q_in:  # the query is computed from this: NaN in, NaN out; the other heads stay clean
                buf, at = c.nan_q_in
                _host(c.prog, buf)[at] = np.nan
            else:
                _host(c.prog, o["q"])[o["q_off"] + NAN_QUERY * o["q_cs"] + r * o.get("q_rs", 1)] = np.nan
            continue
        cols = dead if variant == "masked" else [dead[c.inf_col]]
        if variant == "inf_k":  # open the column for every query the causal part lets through
            m = _host(c.prog, o["mask"])
            for qi in range(sq):
                if cols[0] <= skv - sq + qi:
                    m[o["mask_off"] + qi * o["mask_cs"] + cols[0] * o["mask_rs"]] = 0
        if op.kind == "attention_kvq":  # the block scales carry the poison; the int8 bytes are arbitrary anyway
            bpc = dh // o["block_size"]
            for buf, start, vals in ((o["k"], o["k_col_start"], None), (o["v"], o["v_col_start"], POISON_V)):
                sc = _host(c.prog, buf)[o["n_cols"] * dh // 4:]
                for s in cols:
                    for b in range(bpc):
                        sc[(start + s) * bpc + b] = (np.nan if variant == "masked" else np.inf) if vals is None else vals[(s + b) % 3]
            continue
        k, v = _host(c.prog, o["k"]), _host(c.prog, o["v"])
        for s in cols:
            k[o["k_off"] + s * o["k_cs"] + r * o["k_rs"]] = np.nan if variant == "masked" else np.inf
            v[o["v_off"] + s * o["v_cs"] + r * o["v_rs"]] = POISON_V[(r + s) % 3]


def expected_of_variant(c, variant, clean_outs):
    """what a variant must give, from the clean run's outputs (one array per c.outs)"""
    want = [w.copy() for w in clean_outs]
    if variant == "nan_q":
        if c.nan_q_zero:
            for w, b in zip(want, c.outs):
                w[c.nan_q_zero[b]] = 0
        else:
            for w, op in zip(want, c.attention_ops()):
                o = op.f
                w[o["dst_off"] + NAN_QUERY * o["dst_cs"] + np.arange(o["d_head"]) * o.get("dst_rs", 1)] = 0
    return want


# ── the float64 side ───────────────────────────────────────────────────────────────────────────────────────────────────────

def float64_attention(op, bufs, seq_kv=None):
    """softmax(Q K^T scale + mask) V in float64 from the op's own strides over `bufs` (buffer index -> flat f32 array);
    a query with no finite score gives zeros. Returns [seq_q, d_head]."""
    o = op.f
    dh, sq, skv = o["d_head"], o["seq_q"], seq_kv or o["seq_kv"]
    r, s, qi = np.arange(dh), np.arange(skv), np.arange(sq)
    q = bufs[o["q"]][o["q_off"] + qi[:, None] * o["q_cs"] + r[None, :] * o.get("q_rs", 1)].astype(np.float64)
    if op.kind == "attention_kvq":
        def deq(buf, start):
            n = o["n_cols"] * dh
            data = bufs[buf][:n // 4].view(np.int8).reshape(o["n_cols"], dh).astype(np.float64)
            sc = bufs[buf][n // 4:].reshape(o["n_cols"], dh // o["block_size"]).astype(np.float64)
            return (data * np.repeat(sc, o["block_size"], axis=1))[start:start + skv]
        k, v = deq(o["k"], o["k_col_start"]), deq(o["v"], o["v_col_start"])
    else:
        k = bufs[o["k"]][o["k_off"] + s[:, None] * o["k_cs"] + r[None, :] * o["k_rs"]].astype(np.float64)
        v = bufs[o["v"]][o["v_off"] + s[:, None] * o["v_cs"] + r[None, :] * o["v_rs"]].astype(np.float64)
    sc = q @ k.T * np.float64(f32(o["scale"]))
    if o["has_mask"]:
        sc = sc + bufs[o["mask"]][o["mask_off"] + qi[:, None] * o["mask_cs"] + s[None, :] * o["mask_rs"]].astype(np.float64)
    sc[~np.isfinite(sc)] = -np.inf
    m = sc.max(axis=1, keepdims=True)
    w = np.where(np.isfinite(sc), np.exp(sc - np.where(np.isfinite(m), m, 0)), 0)
    den = w.sum(axis=1, keepdims=True)
    return np.where(den > 0, w @ v / np.where(den > 0, den, 1), 0)


def gather_out(op, dst):
    """[seq_q, d_head] view of what the op stored in its destination buffer"""
    o = op.f
    return dst[o["dst_off"] + np.arange(o["seq_q"])[:, None] * o["dst_cs"] + np.arange(o["d_head"])[None, :] * o.get("dst_rs", 1)]


def run_case(be, c, seq_kvs=None):
    """c.prog on `be` (oracle or HIP): the destination buffers after the compile-time seq_kv and after each refresh.
    Returns ([[array per c.outs] per seq_kv], plan text or None)."""
    h = be.compileProgram(c.prog)
    assert h, getattr(be, "last_error", lambda: "compile failed")()
    try:
        res = []
        for n in (None,) + tuple(seq_kvs or ()):
            if n is not None:
                be.refreshProgram(h, [o.with_(seq_kv=n) if o.kind in ("attention", "attention_kvq") else o for o in c.prog.ops])
            outs = [ProgramIO(b, np.zeros(c.prog.buffer_sizes[b], f32)) for b in c.outs]
            be.executeProgram(h, [], outs)
            res.append([o.host for o in outs])
        return res, (be.planText(h) if hasattr(be, "planText") else None)
    finally:
        be.freeProgram(h)
