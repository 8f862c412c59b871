"""CPU tests of the repetition / presence / frequency penalties of seeded sampling (include/zgml_hip.h: the tail of zgml_sampling).
The rule is zgml_amd/csrc/sample.h — sample_penalize, sample_window_count, sample_window_span, the functions the kernels call —
and the refusals are zgml_amd/csrc/sample_params.h, the function the runtime calls; both reached through
tests/cpp/penalty_probe.cpp (g++ -ffp-contract=off):

1. sample_penalize against a numpy float32 restatement, to the bit, special values included.
2. The window's counts against collections.Counter over the slice the contract names.
3. With every penalty neutral the penalised pick is the existing pick (tests/cpp/sample_probe.cpp), for every position tried; and
   the two cases that tell penalising before the selection from re-weighting its result.
4. The probe's stand-alone program under AddressSanitizer + UBSan.
5. The refusals that are pure host logic; sizeof / offsets of the new fields against the ctypes mirror."""
import ctypes as C
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi
from tests.test_sample_host import c_candidates, c_sample

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libpenalty_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "penalty_probe.cpp", ROOT / "zgml_amd" / "csrc" / "sample.h", ROOT / "zgml_amd" / "csrc" / "sample_params.h",
        ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
f32 = np.float32
S = capi.SamplingC.of
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
    lib.c_penalize.argtypes, lib.c_penalize.restype = [fl, u32, fl, fl, fl], fl
    lib.c_window_counts.argtypes, lib.c_window_counts.restype = [vp, u32, vp], None
    lib.c_window_span.argtypes, lib.c_window_span.restype = [u32, u32, u32, C.POINTER(u32)], u32
    lib.c_penalized_logits.argtypes, lib.c_penalized_logits.restype = [vp, u32, fl, fl, fl, u32, vp, u32, vp], None
    lib.c_candidates_penalized.argtypes, lib.c_candidates_penalized.restype = [vp, u32, u32, fl, fl, fl, u32, vp, u32, vp], u32
    lib.c_sample_penalized.argtypes, lib.c_sample_penalized.restype = [vp, u32, u32, fl, fl, u64, u32, u32, fl, fl, fl, u32, vp, u32], u32
    lib.c_penalty_check.argtypes, lib.c_penalty_check.restype = [C.POINTER(capi.SamplingC), C.c_int, u32, u32, C.POINTER(fl), C.POINTER(u32)], C.c_char_p
    _lib = lib
    return lib


def _recent(recent):
    r = np.ascontiguousarray(recent, np.uint32)
    return r, (r.ctypes.data if r.size else None), r.size


def c_candidates_penalized(v, sp, recent):
    """the header's candidates for logits v under the capi.SamplingC sp (its penalties and its window length; sp.recent is NOT
    read) behind `recent`: the tokens up to and including the one whose logits these are, oldest first"""
    v = np.ascontiguousarray(v, f32)
    r, rp, rn = _recent(recent)
    out = np.zeros(256, np.uint32)
    k = probe().c_candidates_penalized(v.ctypes.data, v.size, sp.top_k, sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty, sp.penalty_window,
                                       rp, rn, out.ctypes.data)
    return out[:k].tolist()


def c_sample_penalized(v, sp, position, recent):
    """... and the header's token at `position` (what a device pick must equal)"""
    v = np.ascontiguousarray(v, f32)
    r, rp, rn = _recent(recent)
    return int(probe().c_sample_penalized(v.ctypes.data, v.size, sp.top_k, sp.temperature, sp.top_p, sp.seed, sp.stream, position, sp.repeat_penalty,
                                          sp.presence_penalty, sp.frequency_penalty, sp.penalty_window, rp, rn))


def c_penalized_logits(v, sp, recent):
    v = np.ascontiguousarray(v, f32)
    r, rp, rn = _recent(recent)
    out = np.zeros(v.size, f32)
    probe().c_penalized_logits(v.ctypes.data, v.size, sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty, sp.penalty_window, rp, rn, out.ctypes.data)
    return out


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ── 1. the penalty ─────────────────────────────────────────────────────────────────────────────────────────────────────

def np_penalize(v, count, repeat, presence, frequency):
    """the rule restated in numpy float32, one rounded operation per line"""
    v, repeat, presence, frequency = f32(v), f32(repeat), f32(presence), f32(frequency)
    if count == 0:
        return v
    inv_repeat = f32(1.0) / repeat
    with np.errstate(all="ignore"):
        v1 = v * inv_repeat if v > 0 else v * repeat
        v2 = v1 - f32(count) * frequency
        return v2 - presence


def test_penalize_equals_the_numpy_restatement_to_the_bit():
    lib, rng = probe(), np.random.default_rng(7)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.4e38, -3.4e38, 1e-45, -1e-45, 1.17549435e-38]
    values = np.concatenate([np.array(special, f32), (rng.standard_normal(300) * 8).astype(f32), rng.standard_normal(100).astype(f32) * f32(1e-3)])
    counts = [0, 1, 2, 3, 7, 255, 256, 300] + rng.integers(0, 301, 8).tolist()
    n = 0
    for repeat in (0.5, 1.0, 1.1, 2.0):
        for presence, frequency in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.25), (-0.75, 0.1), (0.3, -0.2), (-1.5, -0.05)):
            for count in counts:
                for v in values:
                    got = f32(lib.c_penalize(float(v), int(count), repeat, presence, frequency))
                    want = np_penalize(v, int(count), repeat, presence, frequency)
                    if np.isnan(want):
                        assert np.isnan(got), (v, count, repeat, presence, frequency)
                    else:
                        assert bits(got) == bits(want), (v, count, repeat, presence, frequency, got, want)
                    if count == 0 and not np.isnan(v):
                        assert bits(got) == bits(v)  # untouched, the sign of a zero included
                    n += 1
    assert n > 100000
    # a NaN with count 0 comes back with its own bits (ctypes passes a float through a double: the quiet NaN keeps its payload)
    assert np.isnan(lib.c_penalize(float("nan"), 0, 1.1, 0.5, 0.5))


# ── 2. the window ──────────────────────────────────────────────────────────────────────────────────────────────────────

def window_counts(win):
    win = np.ascontiguousarray(win, np.uint32)
    out = np.zeros(max(win.size, 1), np.uint32)
    probe().c_window_counts(win.ctypes.data if win.size else None, win.size, out.ctypes.data)
    return out[:win.size].tolist()


def counts_as_dict(win):
    got = {}
    for t, c in zip(win, window_counts(win)):
        if c:
            assert t not in got  # every distinct token is reported once, at its first entry
            got[int(t)] = c
    first = {}
    for i, t in enumerate(win):
        first.setdefault(int(t), i)
    assert [i for i, c in enumerate(window_counts(win)) if c] == sorted(first.values())
    return got


@pytest.mark.parametrize("W", [1, 2, 255, 256])
def test_window_counts_equal_counter_over_the_contracts_slice(W):
    lib, rng = probe(), np.random.default_rng(W)
    for lo, P in [(0, 0), (0, 1), (0, W - 1), (0, W), (0, 299), (5, 5), (5, 5 + W - 2), (5, 5 + W - 1), (5, 5 + W), (250, 300), (100, 600)]:
        if P < lo:
            continue
        toks = rng.integers(0, 12, P + 1)  # the token at every position 0 .. P (a small alphabet: repeats)
        first = C.c_uint32(0)
        m = lib.c_window_span(P, lo, W, C.byref(first))
        assert (first.value, m) == (max(lo, P + 1 - W), P - max(lo, P + 1 - W) + 1), (lo, P)  # positions max(lo, P + 1 - W) .. P
        win = toks[first.value:P + 1]
        assert counts_as_dict(win) == dict(Counter(int(t) for t in win)), (lo, P)
    assert lib.c_window_span(3, 4, W, C.byref(first)) == 0  # nothing known yet
    # one token W times
    assert window_counts([9] * W) == [W] + [0] * (W - 1)
    assert counts_as_dict(list(range(W))) == {t: 1 for t in range(W)}


def test_sample_form_reads_the_last_w_entries_and_ignores_tokens_behind_n():
    rng = np.random.default_rng(5)
    n = 50
    v = rng.standard_normal(n).astype(f32)
    hist = rng.integers(0, 70, 400).tolist()  # (tokens 50 .. 69 are >= n)
    assert any(t >= n for t in hist[-4:] + hist[-255:])
    for W in (1, 2, 4, 255, 256):
        sp = S(0.8, 40, 0.95, repeat_penalty=1.3, presence_penalty=0.25, frequency_penalty=0.5, penalty_window=W)
        for cut in (0, 1, W - 1, W, W + 1, 400):
            recent = hist[len(hist) - cut:] if cut else []
            want = v.copy()
            for t, c in Counter(recent[-W:]).items():
                if t < n:
                    want[t] = np_penalize(v[t], c, 1.3, 0.25, 0.5)
            got = c_penalized_logits(v, sp, recent)
            assert np.array_equal(bits(got), bits(want)), (W, cut)


# ── 3. neutral penalties; before, not after, the selection ─────────────────────────────────────────────────────────────

def test_neutral_penalties_are_the_existing_pick():
    rng = np.random.default_rng(21)
    for n in (1, 257, 1000):
        v = rng.standard_normal(n).astype(f32)
        v[rng.integers(0, n, 3)] = [np.nan, -np.inf, -0.0]
        recent = rng.integers(0, n, 300).tolist()
        base = S(0.8, 40, 0.95, seed=77, stream=2)
        for kw in (dict(), dict(penalty_window=64), dict(repeat_penalty=1.0, penalty_window=256), dict(repeat_penalty=0.0, presence_penalty=0.0, penalty_window=4)):
            sp = S(0.8, 40, 0.95, seed=77, stream=2, **kw)
            assert c_candidates_penalized(v, sp, recent) == c_candidates(v, 40)
            for pos in range(64):
                assert c_sample_penalized(v, sp, pos, recent) == c_sample(v, base, pos), (n, kw, pos)
        assert np.array_equal(bits(c_penalized_logits(v, S(penalty_window=8), recent)), bits(v))


def push_out_and_pull_in(n=1000):
    """(v, push-out case, pull-in case): a descending ramp, v[i] = 8 - i / 64, so the raw rank of token i is i"""
    v = (8.0 - np.arange(n) / 64.0).astype(f32)
    push = (S(0.8, 1, 1.0, repeat_penalty=2.0, penalty_window=4), [0])                              # the raw maximum, halved: 4 < v[1]
    pull = (S(0.8, 40, 1.0, repeat_penalty=0.5, presence_penalty=-1.0, penalty_window=4), [300])    # raw rank 300: 3.3125 -> 7.625
    return v, push, pull


def test_penalties_act_before_the_selection():
    v, (sp, recent), (sp2, recent2) = push_out_and_pull_in()
    assert c_candidates(v, 1) == [0]
    assert c_candidates_penalized(v, sp, recent) == [1]  # re-weighting the one raw candidate could only give [0]
    assert all(c_sample_penalized(v, sp, pos, recent) == 1 for pos in range(16))
    assert 300 not in c_candidates(v, 256)  # below the 256 largest: no re-weighting of the candidate list can reach it
    cand = c_candidates_penalized(v, sp2, recent2)
    assert len(cand) == 40 and cand.index(300) == 25  # 7.625 = v[24]: right behind token 24 (the lower index first among equals)
    assert cand == list(range(25)) + [300] + list(range(25, 39))


# ── 4. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "penalty_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPENALTY_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "penalty_probe ok" in r.stdout, r.stdout + r.stderr


# ── 5. the boundary ────────────────────────────────────────────────────────────────────────────────────────────────────

NEW_FIELDS = ["repeat_penalty", "presence_penalty", "frequency_penalty", "penalty_window", "recent", "n_recent"]


def test_new_fields_layout_matches_c(tmp_path):
    fields = [n for n, _ in capi.SamplingC._fields_]
    assert fields[-len(NEW_FIELDS):] == NEW_FIELDS  # appended: every earlier field keeps its offset
    body = 'printf("%zu\\n", sizeof(zgml_sampling));' + "".join(f'printf("%zu\\n", offsetof(zgml_sampling, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.SamplingC)] + [getattr(capi.SamplingC, f).offset for f in fields]
    assert capi.SamplingC.seed.offset == 40 and capi.SamplingC.repeat_penalty.offset == 48  # the fields of before, where they were


def test_of_defaults_to_off_and_slices_recent():
    sp = S(0.8, 40, 0.95, seed=1)
    assert (sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty, sp.penalty_window, sp.n_recent) == (0.0, 0.0, 0.0, 0, 0) and not sp.recent
    sp = S(repeat_penalty=1.1, penalty_window=4, recent=list(range(100)))
    assert sp.n_recent == 4 and [sp.recent[i] for i in range(4)] == [96, 97, 98, 99]
    sp = S(repeat_penalty=1.1, penalty_window=4, recent=[5])
    assert sp.n_recent == 1 and sp.recent[0] == 5
    sp = S(repeat_penalty=1.1, penalty_window=4, recent=[])
    assert sp.n_recent == 0 and bool(sp.recent)  # (an empty history is still an array)


def check(sp, form, vocab=100, start_pos=50):
    """-> (why refused or None, repeat as the rule reads it, active)"""
    repeat, active = C.c_float(-1.0), C.c_uint32(7)
    why = probe().c_penalty_check(C.byref(sp), form, vocab, start_pos, C.byref(repeat), C.byref(active))
    return (why.decode() if why else None), repeat.value, active.value


SAMPLE, LOOP, SPEC = 0, 1, 2


def test_refusals_of_the_penalty_fields():
    nan, inf = float("nan"), float("inf")
    for form in (SAMPLE, LOOP, SPEC):
        # off: an all-zero tail, and a window without a penalty
        assert check(S(), form) == (None, 1.0, 0)
        assert check(S(penalty_window=64), form) == (None, 1.0, 0)
        assert check(S(repeat_penalty=1.0, penalty_window=64), form) == (None, 1.0, 0)
        # on: any one penalty
        for kw in (dict(repeat_penalty=1.1), dict(repeat_penalty=0.5), dict(presence_penalty=-0.5), dict(frequency_penalty=0.25)):
            why, repeat, active = check(S(penalty_window=1, **kw), form)
            assert why is None and active == 1 and repeat == f32(kw.get("repeat_penalty", 1.0))
        assert check(S(penalty_window=256, presence_penalty=1.0), form)[0] is None
        # refused
        for kw in (dict(repeat_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5)):
            assert "penalty_window > 0" in check(S(**kw), form)[0]
        assert "at most 256" in check(S(penalty_window=257), form)[0]
        assert "at most 256" in check(S(repeat_penalty=1.1, penalty_window=257), form)[0]
        for kw in (dict(repeat_penalty=nan), dict(repeat_penalty=inf), dict(repeat_penalty=-0.5), dict(presence_penalty=nan), dict(presence_penalty=-inf),
                   dict(frequency_penalty=nan), dict(frequency_penalty=inf)):
            assert "finite" in check(S(penalty_window=4, **kw), form)[0], kw
        sp = S(repeat_penalty=1.1, penalty_window=4)
        sp.n_recent = 3  # recent = NULL
        assert "without the recent tokens" in check(sp, form)[0]
    with_recent = S(repeat_penalty=1.1, penalty_window=4, recent=[1, 2, 99])
    assert check(with_recent, SAMPLE)[0] is None and check(with_recent, LOOP)[0] is None
    assert "recent must be NULL" in check(with_recent, SPEC)[0]
    assert "recent must be NULL" in check(S(repeat_penalty=1.1, penalty_window=4, recent=[]), SPEC)[0]
    # the loops: every recent token is a token of the vocabulary, and lies behind start_pos
    assert "out of range" in check(with_recent, LOOP, vocab=99)[0]
    assert check(with_recent, SAMPLE, vocab=0)[0] is None  # (zgml_hip_sample ignores a token >= n instead)
    assert check(with_recent, LOOP, start_pos=3)[0] is None
    assert "exceeds start_pos" in check(with_recent, LOOP, start_pos=2)[0]
