"""CPU tests of constrained decoding (include/zgml_hip.h: zgml_token_dfa, zgml_hip_constraint_create, zgml_hip_program_set_constraint).
The rule is zgml_amd/csrc/sample.h — constraint_allowed, constraint_advance, sample_real_keys, the functions the kernels call — and
the refusals are zgml_amd/csrc/sample_params.h, the functions the runtime calls; both reached through
tests/cpp/constraint_probe.cpp (g++ -ffp-contract=off):

1. The candidate list and the pick under a mask against the float64 model tests/constraint_model.py. The model may set a case
   aside only under tests/sample_model.py's MARGIN rule, and at most 2 % of the cases — asserted from the model alone, before the
   header is asked.
2. The state's advance over random walks; fewer allowed tokens than top_k; one allowed token; none; -inf / NaN / signed zeros
   among the allowed tokens; penalties with a mask.
3. The refusals that are pure host logic; sizeof / offsets of zgml_token_dfa against the ctypes mirror.
4. The probe's stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi
from tests import constraint_model as CM
from tests.test_sample_host import c_candidates, c_sample, probe as sample_probe

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libconstraint_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "constraint_probe.cpp", ROOT / "zgml_amd" / "csrc" / "sample.h", ROOT / "zgml_amd" / "csrc" / "sample_params.h",
        ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
f32, u16 = np.float32, np.uint16
S = capi.SamplingC.of
FORBIDDEN = 0xFFFF
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", *FLAGS, "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u32, u64, fl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib.c_constraint_allowed.argtypes, lib.c_constraint_allowed.restype = [vp, u32, vp, u32, u32], C.c_int
    lib.c_constraint_advance.argtypes, lib.c_constraint_advance.restype = [vp, u32, vp, u32, u32], u32
    lib.c_real_keys.argtypes, lib.c_real_keys.restype = [vp, u32], u32
    lib.c_constraint_candidates.argtypes, lib.c_constraint_candidates.restype = [vp, u32, u32, fl, fl, fl, u32, vp, u32, vp, vp, u32, u32, vp], u32
    lib.c_constraint_sample.argtypes = [vp, u32, u32, fl, fl, u64, u32, u32, fl, fl, fl, u32, vp, u32, vp, vp, u32, u32, C.POINTER(u32)]
    lib.c_constraint_sample.restype = C.c_int64
    lib.c_constraint_pick.argtypes, lib.c_constraint_pick.restype = [vp, u32, u32, fl, fl, fl, vp, vp, u32, u32, C.POINTER(u32)], C.c_int64
    lib.c_constraint_check.argtypes, lib.c_constraint_check.restype = [C.POINTER(capi.TokenDfaC)], C.c_char_p
    lib.c_constraint_attach_check.argtypes, lib.c_constraint_attach_check.restype = [u32] * 6, C.c_char_p
    _lib = lib
    return lib


class Dfa:
    """an automaton as the probe and the device take it: class_of uint16[vocab], next uint16[n_states, n_classes]"""

    def __init__(self, class_of, next_table):
        self.class_of = np.ascontiguousarray(class_of, u16)
        self.next = np.ascontiguousarray(next_table, u16)
        self.n_states, self.n_classes = self.next.shape

    def allowed(self, state):
        return CM.allowed(self.class_of, self.next, state)

    def advance(self, state, token):
        return CM.advance(self.class_of, self.next, state, token)


def _recent(recent):
    r = np.ascontiguousarray([] if recent is None else recent, np.uint32)
    return r, (r.ctypes.data if r.size else None), r.size


def c_constraint_candidates(v, sp, recent, dfa, state):
    """the header's candidates for logits v under the capi.SamplingC sp (its penalties and window length; sp.recent is NOT read)
    behind `recent` in `state` of `dfa` (None: no constraint)"""
    v = np.ascontiguousarray(v, f32)
    r, rp, rn = _recent(recent)
    out = np.zeros(256, np.uint32)
    cls, nxt, nc = (dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes) if dfa else (None, None, 0)
    k = probe().c_constraint_candidates(v.ctypes.data, v.size, sp.top_k, sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty, sp.penalty_window,
                                        rp, rn, cls, nxt, nc, state, out.ctypes.data)
    return out[:k].tolist()


def c_constraint_sample(v, sp, position, recent, dfa, state):
    """... and the header's (token, state afterwards) at `position`: what a device pick must equal. Token -1: nothing is allowed"""
    v = np.ascontiguousarray(v, f32)
    r, rp, rn = _recent(recent)
    after = C.c_uint32(0)
    cls, nxt, nc = (dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes) if dfa else (None, None, 0)
    tok = probe().c_constraint_sample(v.ctypes.data, v.size, sp.top_k, sp.temperature, sp.top_p, sp.seed, sp.stream, position, sp.repeat_penalty,
                                      sp.presence_penalty, sp.frequency_penalty, sp.penalty_window, rp, rn, cls, nxt, nc, state, C.byref(after))
    return int(tok), int(after.value)


def random_dfa(rng, vocab, n_states=5, n_classes=7, forbid=0.5):
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(u16)
    nxt[rng.random((n_states, n_classes)) < forbid] = FORBIDDEN
    return Dfa(rng.integers(0, n_classes, vocab), nxt)


# ── 1. candidates and pick against the model ───────────────────────────────────────────────────────────────────────────

def mask_cases():
    rng = np.random.default_rng(4242)
    cases = []
    for k in (1, 2, 5, 40, 256):
        for T in (0.25, 0.8, 1.5):
            for top_p in (0.5, 0.95, 1.0):
                for spread in (0.5, 4.0):
                    for _ in range(12):
                        n = int(rng.choice([5, 40, 300, 2000]))
                        v = (rng.standard_normal(n) * spread).astype(f32)
                        if rng.random() < 0.3:
                            v = (np.round(v * 4) / 4).astype(f32)  # ties
                        dfa = random_dfa(rng, n, forbid=float(rng.choice([0.2, 0.5, 0.8])))
                        cases.append((v, k, T, top_p, float(rng.integers(0, 1 << 24)) * 2.0 ** -24, dfa, int(rng.integers(0, 5))))
    return cases


def test_candidates_and_pick_under_a_mask_match_the_float64_model():
    cases = mask_cases()
    assert len(cases) >= 1000
    want = [CM.pick(v, k, T, top_p, u, d.class_of, d.next, st) for v, k, T, top_p, u, d, st in cases]
    set_aside = sum(a for _, _, a, _ in want)
    print(f"set aside as ambiguous: {set_aside} of {len(cases)}")
    assert set_aside <= 0.02 * len(cases)  # a condition on the cases, checked before the header is asked
    assert sum(t < 0 for t, _, _, _ in want) >= 5 and sum(t >= 0 for t, _, _, _ in want) >= 900  # both kinds of state occur
    lib, wrong, masked = probe(), [], 0
    for (v, k, T, top_p, u, d, st), (tok, rank, ambiguous, _) in zip(cases, want):
        cand = CM.candidates(v, k, d.class_of, d.next, st).tolist()
        assert c_constraint_candidates(v, S(top_k=k), None, d, st) == cand
        masked += cand != c_candidates(v, k)
        r = C.c_uint32(0)
        got = int(lib.c_constraint_pick(v.ctypes.data, v.size, k, T, top_p, u, d.class_of.ctypes.data, d.next.ctypes.data, d.n_classes, st, C.byref(r)))
        if tok < 0:
            assert got == -1
        elif (got, r.value) != (tok, rank) and not ambiguous:
            wrong.append((k, T, top_p, u, got, tok))
    assert masked >= 0.5 * len(cases)  # the masks do something (a top_k = 1 list changes only when the maximum itself is forbidden)
    assert not wrong, wrong[:5]


def test_no_constraint_is_the_unconstrained_list():
    rng = np.random.default_rng(1)
    for n in (1, 300, 4097):
        v = rng.standard_normal(n).astype(f32)
        for k in (0, 1, 40):
            assert c_constraint_candidates(v, S(top_k=k), None, None, 0) == c_candidates(v, k)


def test_real_keys_counts_the_keys_before_the_pads():
    lib = probe()
    for k0 in (1, 2, 3, 40, 255, 256):
        for real in sorted({0, 1, k0 // 2, max(k0 - 1, 0), k0}):
            keys = np.array([1000 - j for j in range(real)] + [0] * (256 - real), np.uint64)
            assert lib.c_real_keys(keys.ctypes.data, k0) == min(real, k0)


# ── 2. the cases of the contract ───────────────────────────────────────────────────────────────────────────────────────

def test_state_advance_over_random_walks():
    rng, lib = np.random.default_rng(9), probe()
    for vocab, ns, nc in ((50, 5, 7), (1000, 65535, 3), (3000, 4, 8192), (7, 1, 1)):
        d = random_dfa(rng, vocab, ns, nc, forbid=0.1)
        state = int(rng.integers(0, ns))
        for _ in range(200):
            tok = int(rng.integers(0, vocab))
            want = int(d.next[state, d.class_of[tok]])
            assert lib.c_constraint_advance(d.next.ctypes.data, nc, d.class_of.ctypes.data, state, tok) == want
            assert bool(lib.c_constraint_allowed(d.next.ctypes.data, nc, d.class_of.ctypes.data, state, tok)) == (want != FORBIDDEN)
            if want != FORBIDDEN:
                state = want


def two_class_dfa(vocab, allowed_tokens, n_states=2):
    """class 1 = the allowed tokens; state 0 allows class 1 alone and stays; state 1 allows nothing"""
    cls = np.zeros(vocab, u16)
    cls[list(allowed_tokens)] = 1
    nxt = np.full((n_states, 2), FORBIDDEN, u16)
    nxt[0, 1] = 0
    return Dfa(cls, nxt)


def test_fewer_allowed_tokens_than_top_k():
    rng = np.random.default_rng(3)
    v = rng.standard_normal(1000).astype(f32)
    d = two_class_dfa(1000, [17, 400, 999])
    cand = c_constraint_candidates(v, S(top_k=40), None, d, 0)
    assert sorted(cand) == [17, 400, 999] and cand == sorted(cand, key=lambda t: -v[t])
    seen = {c_constraint_sample(v, S(1.5, 40, 1.0, seed=3), pos, None, d, 0)[0] for pos in range(300)}
    assert seen == {17, 400, 999}  # the k of the pick is 3: all three come, nothing else does


def test_one_allowed_token_is_returned_for_every_u():
    rng, lib = np.random.default_rng(4), probe()
    v = rng.standard_normal(500).astype(f32)
    t = int(np.argmin(v))  # the least likely token of the raw row
    d = two_class_dfa(500, [t])
    for u in [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24] + rng.random(50).tolist():
        for top_p in (0.1, 1.0):
            assert lib.c_constraint_pick(v.ctypes.data, v.size, 40, 0.8, top_p, u, d.class_of.ctypes.data, d.next.ctypes.data, 2, 0, None) == t
    assert c_constraint_sample(v, S(0.8, 40, 0.95, seed=1), 7, None, d, 0) == (t, 0)


def test_no_allowed_token_gives_no_candidates_and_no_token():
    v = np.arange(100, dtype=f32)
    d = two_class_dfa(100, [5])
    assert c_constraint_candidates(v, S(top_k=40), None, d, 1) == []
    assert c_constraint_sample(v, S(0.8, 40, 0.95, seed=1), 0, None, d, 1) == (-1, 1)  # the state stays


def test_an_allowed_minus_inf_or_nan_stays_a_candidate_and_is_never_picked():
    v = np.full(600, 9.0, f32)
    allowed = [10, 300, 301, 599]
    v[allowed] = [-np.inf, 1.0, np.nan, 0.5]
    d = two_class_dfa(600, allowed)
    assert c_constraint_candidates(v, S(top_k=40), None, d, 0) == [300, 599, 10, 301]  # p = 0 and a rank each: -inf and NaN == -inf, the lower index first
    for pos in range(300):
        for top_p in (0.95, 1.0):
            assert c_constraint_sample(v, S(1.5, 40, top_p, seed=2), pos, None, d, 0)[0] in (300, 599)
    # ... and alone they are what there is: the rank that a row of these two logits gives without a constraint (all p = 0: the fall-back)
    d2 = two_class_dfa(600, [10, 301])
    sp = S(1.5, 40, 1.0, seed=2)
    assert c_constraint_sample(v, sp, 0, None, d2, 0)[0] == [10, 301][c_sample(v[[10, 301]], sp, 0)]


def test_signed_zero_ties_among_allowed_tokens():
    v = np.full(400, 1.0, f32)
    allowed = [3, 50, 51, 399]
    v[allowed] = [-0.0, 0.0, -0.0, 0.0]
    d = two_class_dfa(400, allowed)
    assert c_constraint_candidates(v, S(top_k=40), None, d, 0) == allowed  # -0 == +0: the index decides
    assert c_constraint_candidates(v, S(top_k=2), None, d, 0) == [3, 50]
    assert CM.candidates(v, 40, d.class_of, d.next, 0).tolist() == allowed


def test_penalties_and_mask_match_the_model():
    rng = np.random.default_rng(77)
    pen = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, penalty_window=8)
    changed = 0
    for case in range(60):
        n = int(rng.choice([40, 300, 2000]))
        v = (rng.standard_normal(n) * 3).astype(f32)
        d = random_dfa(rng, n, forbid=0.5)
        st = int(rng.integers(0, 5))
        top = np.argsort(-v)[:6].tolist()
        recent = [int(t) for t in rng.choice(top + [n + 3], 12)]  # repeats of the largest logits, allowed or not; one token >= n
        sp = S(0.8, 40, 0.95, seed=case, **pen)
        pv = CM.penalized(v, recent, 8, 1.3, 0.5, 0.25)
        want = CM.candidates(pv, 40, d.class_of, d.next, st).tolist()
        assert c_constraint_candidates(v, sp, recent, d, st) == want
        changed += want != CM.candidates(v, 40, d.class_of, d.next, st).tolist()
        # the order of mask and penalty does not matter: penalised values, then the mask == the mask over penalised values
        u = float(sample_probe().sp_uniform(case, 0, 11))
        tok, rank, ambiguous, after = CM.pick(pv, 40, 0.8, 0.95, u, d.class_of, d.next, st)
        got = c_constraint_sample(v, sp, 11, recent, d, st)
        assert ambiguous or got == (tok, after)
    assert changed >= 30  # the penalties do something under the mask


# ── 3. the refusals, the boundary ──────────────────────────────────────────────────────────────────────────────────────

def check(class_of, next_table, **sizes):
    why = probe().c_constraint_check(C.byref(capi.TokenDfaC.of(class_of, next_table, **sizes)))
    return why.decode() if why else None


def test_create_refusals_are_pure_host_logic():
    cls, nxt = np.array([0, 1, 2, 1], u16), np.array([[0, 1, FORBIDDEN], [1, 1, 0]], u16)
    assert check(cls, nxt) is None
    assert check(cls, np.full((65535, 1), FORBIDDEN, u16), n_classes=1, vocab=1) is None and check(np.zeros(3, u16), np.zeros((1, 8192), u16)) is None  # the limits themselves
    assert "class" in check(np.array([0, 1, 3, 1], u16), nxt)
    assert "next state" in check(cls, np.array([[0, 2, FORBIDDEN], [1, 1, 0]], u16))
    assert "n_states" in check(cls, nxt, n_states=0) and "n_states" in check(cls, nxt, n_states=65536)
    assert "n_classes" in check(cls, nxt, n_classes=0) and "n_classes" in check(cls, nxt, n_classes=8193)
    assert "vocab" in check(cls, nxt, vocab=0)
    d = capi.TokenDfaC.of(cls, nxt)
    d.next = None
    assert b"NULL" in probe().c_constraint_check(C.byref(d)) and b"NULL" in probe().c_constraint_check(None)


def test_attach_refusals_are_pure_host_logic():
    att = probe().c_constraint_attach_check  # (automaton's vocab, its n_states, program's vocab, sequences, seq, state)
    assert att(512, 5, 512, 1, 0, 4) is None and att(512, 5, 512, 3, 2, 0) is None
    assert b"vocab" in att(512, 5, 513, 1, 0, 0)
    assert b"seq" in att(512, 5, 512, 1, 1, 0) and b"seq" in att(512, 5, 512, 3, 3, 0)
    assert b"state" in att(512, 5, 512, 1, 0, 5)


def test_token_dfa_layout_matches_c(tmp_path):
    fields = [n for n, _ in capi.TokenDfaC._fields_]
    body = 'printf("%zu\\n", sizeof(zgml_token_dfa));' + "".join(f'printf("%zu\\n", offsetof(zgml_token_dfa, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.TokenDfaC)] + [getattr(capi.TokenDfaC, f).offset for f in fields]


def test_sampling_keeps_its_size_and_the_entry_points_are_exported():
    assert C.sizeof(capi.SamplingC) == 80  # no field was added for the constraint
    lib = capi.load_hip()
    for name in ("zgml_hip_constraint_create", "zgml_hip_constraint_free", "zgml_hip_program_set_constraint", "zgml_hip_program_constraint_state"):
        assert name in capi.HIP_SYMBOLS and hasattr(lib, name)


# ── 4. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "constraint_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DCONSTRAINT_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "constraint_probe ok" in r.stdout, r.stdout + r.stderr
