"""Named cases for the fused decode attention (zgml_amd/csrc/attention_decode.h attention_decode_body) on every instantiation the
launchers reach, at the context lengths where its loop, its wave merge and its key-range split change shape.
tests/test_decode_attention_cases_host.py pins the table on the CPU (coverage from the restated rules, the float64 reference
against the oracle, the poison on the oracle itself), tests/test_hip_decode_attention.py runs the device.

A case is one kv group as the LLaMA lowering emits it (tests/plan_cases.py decode_group): two heads (one case: three) over one kv
head, so the second head is not the column's owner; per head rope q -> attention -> row store, plus rope k -> K store and V store
(f32 KV: slice_assign, int8 KV: kvq_store / attention_kvq with column starts 0 and block 32). The program is compiled once with
seq_kv = max_kv (the caches hold max_kv columns; the split policy sees that bound) and every `Step` is reached with refreshProgram
(store column and seq_kv together), in ascending order of seq_kv. Before each step the mask row, both destinations (-7 sentinels)
and both caches are uploaded: every cache column at or behind the step's seq_kv is NaN (f32 KV: the rows; int8 KV: the block
scales), so the kernel's clamped loads and its `t < k_end` tests must keep them out of the result.

Inputs: standard_normal f32 for the projections and the f32 caches, a real rotation in the cos|sin row, scale = d_head ** -0.5;
int8 caches as attention_cases._kvq_case draws them (bytes in -127..127, scales uniform in 0.004..0.02). The new column comes from
standard-normal projections, so every block maximum is O(1): the 0 * inf clamp corner of kvq.h is not met.

The launcher and kernel rules the lengths were chosen by are restated here, each with the lines it restates:
  decode_form   kernels_generic.hip launch_attention_decode_batch (which <LPK, KVQ, BLOCK> a d_head / cache form / forced block
                takes), attention_decode.h:290-296 (Q16, LPKM, KPW, U) and :378-382 (keys per wave, most waves)
  rounds        attention_decode.h:378-382 and the two loops (:575-584, :634-652): NW, step_keys, rounds, live unrolled rows
  place         the key index arithmetic of the loads and of `step` / `scores`: key -> (round, unrolled row, wave, slot)
  attn_split    plan.hip attn_split_for: S <= 16, <= max_kv / min_keys, min_keys >= 32, <= 256 / heads workgroups
  split         attention_decode.h:361-373: n_active, chunk, the key ranges

Bars. The roped q / k and both caches are claimed bit-equal to the op-by-op plan (attention_decode.h:32-34, :158-161;
plan.hip decode_attention), which is pinned bit-equal to the oracle: equal bits. The head outputs and their row-store copies are
held to ATOL = 2e-5 absolute against float64 attention over those oracle-equal buffers (the project's attention bar:
tests/test_hip_attention_routes.py, tests/test_hip_conformance.py); inputs and outputs are O(1).
The Q16 forms (int8 KV, d_head >= 128) compute their weights as __expf(x) = v_exp_f32(x * log2(e)), x = score - max <= 0: the
product rounds once (u = 2^-24, and log2(e) itself carries u), which moves the result by |x| * 2u relative, and v_exp_f32 adds
one ulp (2u): a weight is off by at most 2u (|x| + 1) relative. A softmax average with weights off by eps_i moves by at most
2 max|V| sum(eps_i w_i) / sum(w_i) <= 4u (X + 1) max|V| with X the largest |score - max| of a live key. At X = 12 and
max|V| = 2.6 (127 * 0.02) that is 8e-6, inside ATOL: the Q16 forms are held to the same bar (measured margins:
profiles/r21_decode_attention_parity.txt)."""
from dataclasses import dataclass, field

import numpy as np

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO
from tests.attention_cases import POISON_V, SENTINEL
from tests.plan_cases import decode_group

f32 = np.float32
ATOL = 2e-5
ORACLE_ATOL = 2e-6        # tests/test_attention_cases_host.py: the oracle's attention against float64
MIN_KEYS, SPLIT_MAX_KV = 32, 544
P, CS, QR, KR, KC, VC, MASK, AO, O = range(9)   # plan_cases.decode_group's buffers
F32_D_HEADS, KVQ_D_HEADS, SPLIT_D_HEADS = (8, 16, 32, 64, 128, 256), (32, 64, 128, 256), (64, 128)
FORCED = {256: 64, 1024: 128}   # ZGML_HIP_ATTN_DECODE_BLOCK -> the d_head whose default it overrides


# ── the restated rules ─────────────────────────────────────────────────────────────────────────────────────────────────────

@dataclass(frozen=True)
class Form:
    d_head: int
    kvq: bool
    block: int            # threads of the workgroup
    lpk: int              # lanes per key of the ropes, the stores and the merges
    q16: bool             # int8 KV with 16 dims per lane in the key loop
    lpkm: int             # lanes per key of the key loop
    kpw: int              # keys a wave streams per load instruction
    kpw4: int             # key slots of the merges
    u: int                # unrolled rows per step
    keys_per_wave: int    # what one more wave is started for
    max_waves: int

    @property
    def full(self):
        """the last single-round length of one workgroup"""
        return self.max_waves * self.kpw * self.u

    @property
    def tag(self):
        return f"{'q16' if self.q16 else 'kvq' if self.kvq else 'f32'}_dh{self.d_head}_b{self.block}"


def body_form(d_head, kvq, block):
    """attention_decode_body<d_head / 4, kvq, block>: attention_decode.h:290-296, :378-382"""
    lpk = d_head // 4
    q16 = kvq and lpk >= 32
    lpkm = d_head // 16 if q16 else lpk
    kpw, u = 64 // lpkm, 4
    return Form(d_head, kvq, block, lpk, q16, lpkm, kpw, 64 // lpk, u, kpw if q16 else kpw * u, block // 64)


def decode_form(d_head, kvq, block_env=0):
    """kernels_generic.hip launch_attention_decode_batch: int8 KV always 1024 threads; f32 KV 256 threads for d_head 128 unless
    ZGML_HIP_ATTN_DECODE_BLOCK forces a size for d_head 64 / 128. None: no such instantiation."""
    if kvq:
        return body_form(d_head, True, 1024) if d_head in KVQ_D_HEADS else None
    if d_head not in F32_D_HEADS:
        return None
    small = block_env == 256 or (block_env == 0 and d_head == 128)
    return body_form(d_head, False, 256 if small and d_head in (64, 128) else 1024)


def rounds(n_keys, form):
    """(NW, keys_per_iter, step_keys, rounds, live unrolled rows of the last round) of a workgroup that streams n_keys keys"""
    nw = min(max(-(-n_keys // form.keys_per_wave), 1), form.max_waves)
    kpi = form.kpw * nw
    step = kpi * form.u
    n_rounds = 1 if n_keys <= step else -(-n_keys // step)
    rem = n_keys - (n_rounds - 1) * step
    return nw, kpi, step, n_rounds, tuple(j for j in range(form.u) if j * kpi < rem)


def place(t, n_keys, form):
    """(round, unrolled row, wave, slot) that meets key t of a workgroup's n_keys keys: t = base + j * keys_per_iter + w * KPW + slot"""
    _, kpi, step, _, _ = rounds(n_keys, form)
    o = t % step
    return t // step, o // kpi, (o % kpi) // form.kpw, o % form.kpw


def attn_split(max_kv, min_keys, n_heads, want=16, wgs=256):
    """plan.hip attn_split_for: the workgroups per head of a launch whose plan allows max_kv keys (1: no split)"""
    if min_keys == 0 or want <= 1:
        return 1
    S = min(want, max_kv // max(32, min_keys), max(1, wgs // max(n_heads, 1)))
    return max(S, 1)


def split(seq_kv, S, min_keys):
    """(n_active, chunk, [(k_begin, k_end)]) — attention_decode.h:361-373"""
    if S <= 1:
        return 1, seq_kv, [(0, seq_kv)]
    n_active = min(max(seq_kv // max(32, min_keys), 1), S)
    chunk = -(-seq_kv // n_active)
    return n_active, chunk, [(min(c * chunk, seq_kv), min(min(c * chunk, seq_kv) + chunk, seq_kv)) for c in range(n_active)]


def cut_lengths(form):
    """{name: seq_kv} of the stand-alone cuts of one workgroup (split off)"""
    cuts = {"one": 1, "one_wave": form.keys_per_wave, "two_waves": form.keys_per_wave + 1, "full": form.full, "second_round": form.full + 1,
            "two_rounds": form.full + form.keys_per_wave + 1, "three_rounds": 2 * form.full + 1}
    if form.q16:  # the unrolled row j = 1 comes alive
        cuts.update(row0_full=form.max_waves * form.kpw, row1=form.max_waves * form.kpw + 1)
    return cuts


SPLIT_LENGTHS = {"one_active": 63, "two_active": 64, "ragged": 65, "fifteen": 511, "sixteen": 512, "capped": 543}


def fused_positions(form, S, min_keys, max_seq):
    """{name: seq_kv} of a fused launch whose attention part runs `form` with S workgroups per head: the first length at which
    some workgroup needs a second round (and the length before it), 63 / 64 / 65, and the first length with all S active"""
    worst = lambda n: max(rounds(e - b, form)[3] for b, e in split(n, S, min_keys)[2])  # noqa: E731
    two = next((n for n in range(1, max_seq + 1) if worst(n) >= 2), None)
    pos = {"s63": 63, "s64": 64, "s65": 65, "capped": S * max(32, min_keys)}
    if two is not None:
        pos.update(last_single=two - 1, first_two=two)
    return {k: v for k, v in pos.items() if 1 <= v <= max_seq}


# The two fused q / k / v + attention launches (qmatvec.hip qkv_attn_kernel for K <= 2048, qkv_attn_kon_kernel for K-on-lanes
# weights), reached through small llama.Models: name -> (d_model, heads, kv heads, d_ff, layers, threads of the attention body,
# layers that take the fused launch). K-on-lanes (d_model 4096): the first layer's projection computes its rmsnorm itself and
# stays apart (plan.hip fuse_qkv_attention: QMV_PRO_PRENORM only), so those models have two layers and the second one is fused.
FUSED_MODELS = {"smollm": (576, 9, 3, 1536, 1, 1024, 1), "dh128": (2048, 16, 4, 2048, 1, 1024, 1),
                "kon_dh64": (4096, 64, 16, 1024, 2, 256, 1), "kon_dh128": (4096, 32, 8, 1024, 2, 256, 1)}
N_CU = 256  # MI355X: the 1024-thread fused launch keeps one workgroup per CU, its split count shrinks to fit (plan.hip fuse_qkv_attention)


def fused_splits(name, max_seq):
    """workgroups per head of a model's fused launch: attn_split_for, then the residency guard of the 1024-thread form"""
    d_model, n_heads, n_kv, _, _, block, _ = FUSED_MODELS[name]
    S = attn_split(max_seq, MIN_KEYS, n_heads)
    if block == 1024:
        S = max(1, min(S, (N_CU - (n_heads + 2 * n_kv) * (d_model // n_heads) // 16) // n_heads))
    return S


def fused_plan(name, kvq):
    """(body form, S, max_seq, the seq_kv values to check) of a fused model: the cuts of every split count up to the restated one —
    should the residency guard give fewer workgroups per head, their cuts are met too"""
    d_model, n_heads, _, _, _, block, _ = FUSED_MODELS[name]
    form = body_form(d_model // n_heads, bool(kvq), block)
    S = fused_splits(name, 1 << 20)
    max_seq = max(fused_positions(form, S, MIN_KEYS, 1 << 14).values()) + 8
    assert fused_splits(name, max_seq) == S
    check = sorted({n for s in range(1, S + 1) for n in fused_positions(form, s, MIN_KEYS, max_seq).values()})
    return form, S, max_seq, check


# ── the cases ──────────────────────────────────────────────────────────────────────────────────────────────────────────────

@dataclass
class Step:
    name: str
    seq_kv: int
    col: int = None                 # store column (default: seq_kv - 1, the decode position)
    dead: tuple = ()                # keys shut by the mask (besides everything at or behind seq_kv)
    poison: bool = False            # attention_cases' `masked` poison on the dead columns; expected: the step `clean_of`
    clean_of: str = None
    twice: bool = False             # a second execute gives identical bits
    zero: bool = False              # no live key: the outputs are exactly zero
    kills: tuple = None             # (what, index) the dead set is claimed to be, for the host test

    def __post_init__(self):
        if self.col is None:
            self.col = self.seq_kv - 1


@dataclass
class Case:
    name: str
    form: Form
    n_heads: int
    o_rs: int
    max_kv: int
    min_keys: int                  # OPT_ATTN_SPLIT_MIN_KEYS of the case (0: split off)
    block_env: int
    prog: DeviceProgram
    steps: list
    caches: tuple = field(repr=False, default=None)   # the finite K / V cache images every step starts from

    @property
    def S(self):
        return attn_split(self.max_kv, self.min_keys, self.n_heads)

    def attention_ops(self, ops=None):
        return [o for o in (ops or self.prog.ops) if o.kind in ("attention", "attention_kvq")]

    def row_stores(self, ops=None):
        return [o for o in (ops or self.prog.ops) if o.kind == "slice_assign" and o.f["patch_stride"] == 0 and o.f["src"] == AO]

    def ops_for(self, st):
        """the op list refreshed to a step: store column and seq_kv"""
        dh = self.form.d_head
        out = []
        for o in self.prog.ops:
            if o.kind in ("attention", "attention_kvq"):
                o = o.with_(seq_kv=st.seq_kv)
            elif o.kind == "kvq_store":
                o = o.with_(col=st.col)
            elif o.kind == "slice_assign" and o.f["patch_stride"]:
                o = o.with_(dst_offset=st.col * dh)
            out.append(o)
        return out

    def mask_row(self, st):
        m = np.full(self.max_kv, -np.inf, f32)
        m[:st.seq_kv] = 0
        m[list(st.dead)] = -np.inf
        return m

    def cache_images(self, st):
        """K and V cache uploads of a step: NaN at and behind seq_kv, the poison on the dead columns"""
        dh, n = self.form.d_head, self.max_kv
        k, v = self.caches[0].copy(), self.caches[1].copy()
        r = np.arange(dh)
        if self.form.kvq:
            bpc = dh // 32
            ks, vs = k[n * dh // 4:].reshape(n, bpc), v[n * dh // 4:].reshape(n, bpc)
            ks[st.seq_kv:] = np.nan
            vs[st.seq_kv:] = np.nan
            if st.poison:
                for s in st.dead:
                    ks[s] = np.nan
                    vs[s] = POISON_V[(s + np.arange(bpc)) % 3]
        else:
            k2, v2 = k.reshape(n, dh), v.reshape(n, dh)
            k2[st.seq_kv:] = np.nan
            v2[st.seq_kv:] = np.nan
            if st.poison:
                for s in st.dead:
                    k2[s] = np.nan
                    v2[s] = POISON_V[(r + s) % 3]
        return k, v

    def inputs(self, st):
        k, v = self.cache_images(st)
        sizes = self.prog.buffer_sizes
        return [ProgramIO(MASK, self.mask_row(st)), ProgramIO(AO, np.full(sizes[AO], SENTINEL, f32)), ProgramIO(O, np.full(sizes[O], SENTINEL, f32)),
                ProgramIO(KC, k), ProgramIO(VC, v)]

    def written(self):
        """{buffer: indices the ops write} of the two destinations; everything else keeps its sentinel"""
        dh = self.form.d_head
        r = np.arange(dh)
        ao = np.concatenate([o.f["dst_off"] + r for o in self.attention_ops()])
        oo = np.concatenate([o.f["dst_offset"] + r * o.f["dst_row_stride"] for o in self.row_stores()])
        return {AO: ao, O: oo}


def group_ops(dh, n_heads, max_kv, kvq, o_rs):
    """plan_cases.decode_group compiled at the cache's last column; int8 KV: the same group over kvq_store / attention_kvq.
    o_rs: the row stores' destination row stride."""
    hd, pos = dh // 2, max_kv - 1
    if not kvq:
        ops, sizes = decode_group(dh=dh, n_heads=n_heads, pos=pos, max_seq=max_kv)
    else:
        ops = [DeviceOp.rope(QR, P, CS, hd, 1, h * dh, 0, h * dh, 1, dh, dh) for h in range(n_heads)]
        ops += [DeviceOp.rope(KR, P, CS, hd, 1, n_heads * dh, 0, 0, 1, dh, dh),
                DeviceOp.kvq_store(KC, KR, dh, 32, max_kv, 0, 0, pos, 1),
                DeviceOp.kvq_store(VC, P, dh, 32, max_kv, (n_heads + 1) * dh, 0, pos, 1)]
        for h in range(n_heads):
            ops.append(DeviceOp.attention_kvq(AO, QR, KC, VC, MASK, True, dh, 1, pos + 1, dh ** -0.5, 32, max_kv, 0, 0, h * dh, dh, h * dh, dh,
                                              0, 1, max_kv))
            ops.append(DeviceOp.slice_assign(O, AO, dh, 1, h * dh, h * dh, 1, dh, h * dh, 1, dh, 0))
        ce = max_kv * dh // 4 + max_kv * (dh // 32)
        sizes = [(n_heads + 2) * dh, dh, n_heads * dh, dh, ce, ce, max_kv, n_heads * dh + 4, n_heads * dh + 4]
    if o_rs != 1:
        ops = [o.with_(dst_base_offset=o.f["dst_base_offset"] * o_rs, dst_offset=o.f["dst_offset"] * o_rs, dst_row_stride=o_rs,
                       dst_col_stride=dh * o_rs) if o.kind == "slice_assign" and o.f["patch_stride"] == 0 else o for o in ops]
        sizes[O] = n_heads * dh * o_rs + 4
    return ops, sizes


def _case(name, form, steps, max_kv, n_heads=2, o_rs=1, min_keys=0, block_env=0):
    rng = np.random.default_rng(sum(name.encode()) * 7919)
    dh = form.d_head
    ops, sizes = group_ops(dh, n_heads, max_kv, form.kvq, o_rs)
    ang = rng.uniform(0, 3, dh // 2)

    def cache():
        if not form.kvq:
            return rng.standard_normal(max_kv * dh).astype(f32)
        data = rng.integers(-127, 128, max_kv * dh).astype(np.int8)
        return np.concatenate([data.view(f32), rng.uniform(0.004, 0.02, max_kv * (dh // 32)).astype(f32)])
    caches = (cache(), cache())
    ups = [ProgramIO(P, rng.standard_normal(sizes[P]).astype(f32)), ProgramIO(CS, np.concatenate([np.cos(ang), np.sin(ang)]).astype(f32)),
           ProgramIO(QR, np.full(sizes[QR], SENTINEL, f32)), ProgramIO(KR, np.full(sizes[KR], SENTINEL, f32)),
           ProgramIO(KC, caches[0].copy()), ProgramIO(VC, caches[1].copy()), ProgramIO(MASK, np.full(max_kv, -np.inf, f32)),
           ProgramIO(AO, np.full(sizes[AO], SENTINEL, f32)), ProgramIO(O, np.full(sizes[O], SENTINEL, f32))]
    steps = sorted(steps, key=lambda s: s.seq_kv)  # (stable: a variant follows the clean step of its length)
    assert all(s.seq_kv <= max_kv and s.col < max_kv for s in steps)
    return Case(name, form, n_heads, o_rs, max_kv, min_keys, block_env, DeviceProgram(ops, sizes, ups), steps, caches)


def _keys(n, form, pred):
    return tuple(t for t in range(n) if pred(*place(t, n, form)))


def _standalone_steps(form):
    """every cut of one workgroup, and the mask variants placed from the geometry"""
    cuts = cut_lengths(form)
    steps = [Step(k, n) for k, n in cuts.items()]
    full, two = cuts["full"], cuts["two_rounds"]
    steps.append(Step("wave_dead", full, dead=_keys(full, form, lambda r, j, w, s: w == 1), kills=("wave", 1)))
    if form.kpw > 1:  # (one key slot per wave: the slot is the wave)
        steps.append(Step("slot_dead", full, dead=_keys(full, form, lambda r, j, w, s: s == 0), kills=("slot", 0)))
    steps.append(Step("first_round_dead", two, dead=_keys(two, form, lambda r, j, w, s: r == 0), kills=("round", 0)))
    n = cuts["second_round"]
    steps.append(Step("only_new_column", n, dead=tuple(range(n - 1))))
    steps.append(Step("all_dead", n, dead=tuple(range(n)), zero=True))
    return steps


def _split_steps(form, S):
    steps = [Step(k, n, twice=True) for k, n in SPLIT_LENGTHS.items()]
    n = SPLIT_LENGTHS["sixteen"]
    b, e = split(n, S, MIN_KEYS)[2][3]
    steps.append(Step("chunk_dead", n, dead=tuple(range(b, e)), twice=True, kills=("chunk", 3)))
    return steps


def _specs():
    """name -> zero-argument builder"""
    t = {}

    def alone(form, block_env=0, n_heads=2, o_rs=1):
        steps = _standalone_steps(form)
        name = form.tag + ("_three_heads" if n_heads == 3 else "")
        t[name] = lambda: _case(name, form, steps, max(s.seq_kv for s in steps) + 3, n_heads, o_rs, 0, block_env)
    for dh in F32_D_HEADS:  # (d_head 32 carries the three heads, d_head 16 and 128 the strided row store)
        alone(decode_form(dh, False), n_heads=3 if dh == 32 else 2, o_rs=3 if dh in (16, 128) else 1)
    for env, dh in FORCED.items():
        alone(decode_form(dh, False, env), block_env=env)
    for dh in KVQ_D_HEADS:
        alone(decode_form(dh, True), o_rs=2 if dh in (64, 256) else 1)
    for dh in SPLIT_D_HEADS:
        for kvq in (False, True):
            form = decode_form(dh, kvq)
            S = attn_split(SPLIT_MAX_KV, MIN_KEYS, 2)
            steps = _split_steps(form, S)
            if (dh, kvq) in ((64, False), (128, True)):  # the stored column inside chunk 3 of 16
                steps.append(Step("store_in_chunk_3", 512, col=100, twice=True))
            name = form.tag + "_split"
            t[name] = (lambda name=name, form=form, steps=steps, dh=dh:
                       _case(name, form, steps, SPLIT_MAX_KV, 2, 2 if dh == 64 else 1, MIN_KEYS))
    for form in (decode_form(64, False), decode_form(128, True)):  # the store-column variants
        steps = [Step("store_mid", 40, col=5), Step("store_at_seq_kv", 40, col=40), Step("store_behind", 40, col=43)]
        name = form.tag + "_store"
        t[name] = lambda name=name, form=form, steps=steps: _case(name, form, steps, 48)
    for form in (decode_form(64, False), decode_form(64, True), decode_form(128, True)):  # the poison, on a whole dead round
        n = cut_lengths(form)["two_rounds"]
        dead = _keys(n, form, lambda r, j, w, s: r == 0)
        steps = [Step("clean", n, dead=dead, kills=("round", 0)), Step("poisoned", n, dead=dead, poison=True, clean_of="clean")]
        name = form.tag + "_poison"
        t[name] = lambda name=name, form=form, steps=steps, n=n: _case(name, form, steps, n + 3)
    return t


_SPECS = _specs()
CASE_NAMES = tuple(_SPECS)


def build_case(name):
    return _SPECS[name]()


def forced_cases(block_env):
    """the cases that need ZGML_HIP_ATTN_DECODE_BLOCK = block_env (latched per process)"""
    return tuple(n for n in CASE_NAMES if n == decode_form(FORCED[block_env], False, block_env).tag)


DEFAULT_CASES = tuple(n for n in CASE_NAMES if not any(n in forced_cases(env) for env in FORCED))


# ── the float64 side and the runner ────────────────────────────────────────────────────────────────────────────────────────

def float64_heads(c, st, bufs):
    """[n_heads, d_head] float64 attention of a step over `bufs` (buffer -> array after the step; the mask as uploaded)"""
    from tests.attention_cases import float64_attention
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([float64_attention(op, bufs, st.seq_kv)[0] for op in c.attention_ops(c.ops_for(st))])


def live_stats(c, st, bufs):
    """(largest |score - max| over live keys, max |V| over live keys) from the float64 side: what the __expf bound is made of"""
    dh, n = c.form.d_head, c.max_kv
    live = np.isfinite(c.mask_row(st)[:st.seq_kv])
    if not live.any():
        return 0.0, 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        if c.form.kvq:
            def deq(b):
                data = b[:n * dh // 4].view(np.int8).reshape(n, dh).astype(np.float64)
                return data * np.repeat(b[n * dh // 4:].reshape(n, dh // 32).astype(np.float64), 32, axis=1)
            k, v = deq(bufs[KC])[:st.seq_kv], deq(bufs[VC])[:st.seq_kv]
        else:
            k, v = (bufs[b].reshape(n, dh)[:st.seq_kv].astype(np.float64) for b in (KC, VC))
        q = bufs[QR].reshape(c.n_heads, dh).astype(np.float64)
        sc = (q @ k[live].T) * float(f32(dh ** -0.5))
    return float((sc.max(axis=1, keepdims=True) - sc).max()), float(np.abs(v[live]).max())


OUT_BUFS = (QR, KR, KC, VC, AO, O)


def run_steps(be, c, executes=lambda st: 1):
    """c on `be` (oracle or HIP): {step name: {buffer: array}} of OUT_BUFS after each step, and the plan text (None on the oracle).
    A step executed more than once must repeat its first bits."""
    h = be.compileProgram(c.prog)
    assert h, getattr(be, "last_error", lambda: "compile failed")()
    try:
        res = {}
        for st in c.steps:
            be.refreshProgram(h, c.ops_for(st))
            first = None
            for _ in range(executes(st)):
                outs = [ProgramIO(b, np.zeros(c.prog.buffer_sizes[b], f32)) for b in OUT_BUFS]
                be.executeProgram(h, c.inputs(st), outs)
                got = {o.buf_idx: o.host for o in outs}
                if first is None:
                    first = got
                else:
                    assert all(np.array_equal(first[b].view(np.uint32), got[b].view(np.uint32)) for b in OUT_BUFS), f"{c.name} {st.name}: executes differ"
            first[MASK] = c.mask_row(st)
            res[st.name] = first
        return res, (be.planText(h) if hasattr(be, "planText") else None)
    finally:
        be.freeProgram(h)


_oracle_runs = {}


def oracle_run(oracle, name):
    """(case, {step: {buffer: array}}) on the oracle: computed once, shared by the tests that need it, never modified"""
    if name not in _oracle_runs:
        c = build_case(name)
        _oracle_runs[name] = (c, run_steps(oracle.OracleBackend(), c)[0])
    return _oracle_runs[name]
