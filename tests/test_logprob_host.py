"""CPU tests of the log-probability rule (include/zgml_hip.h: zgml_hip_logprobs, the `logprobs` field of zgml_sampling). The rule is
zgml_amd/csrc/sample.h — the functions the kernels of logprob.hip call — reached through tests/cpp/logprob_probe.cpp
(g++ -ffp-contract=off):

1. sample_log against float64 log over [0.5, 2^32).
2. The header against float64 v_t - logsumexp(v) in numpy over crafted vectors, under the derived bar
       |error| <= 1e-5 + 2.4e-7 |v_t - M|:
   summation depth 4 + 2 + 8 + blocks <= 36 roundings of 6e-8 on positive terms: 2.2e-6; sample_exp: 1.9e-7; the result's own
   rounding at |log S| <= 14: 8e-7; sample_log: 1e-7 relative of <= 14; a factor of about 2 over their sum; two roundings of
   6e-8 relative on v_t - M (the subtraction and the result). Measured maximum of |error| - 2.4e-7 |v_t - M| over these vectors:
   4.5e-7.
3. The edges, by bits; the sum of the probabilities; block independence (bits); a permutation across blocks (the bar).
4. The refusals of zgml_amd/csrc/sample_params.h; the word's place in zgml_sampling.
5. The probe's stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "liblogprob_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "logprob_probe.cpp", ROOT / "zgml_amd" / "csrc" / "sample.h", ROOT / "zgml_amd" / "csrc" / "sample_params.h",
        ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
f32 = np.float32
NAN_WORD, NEG_INF_WORD = 0x7FC00000, 0xFF800000
BLOCK = 4096
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 49152, 50001]
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
    lib.lp_log.argtypes, lib.lp_log.restype = [fl], fl
    lib.lp_partials.argtypes, lib.lp_partials.restype = [vp, u64, vp, vp], u32
    lib.lp_logprobs.argtypes, lib.lp_logprobs.restype = [vp, u64, vp, u32, vp], None
    lib.lp_logprob.argtypes, lib.lp_logprob.restype = [vp, u64, u32], fl
    lib.lp_check.argtypes, lib.lp_check.restype = [u64, u64, u64, u32, vp, vp], C.c_char_p
    lib.lp_field_check.argtypes, lib.lp_field_check.restype = [C.c_int, u64], C.c_char_p
    _lib = lib
    return lib


def c_logprobs(v, tokens):
    """the header's log-probabilities of `tokens` under the row v (what a device value must equal, to the bit)"""
    v, t = np.ascontiguousarray(v, f32), np.ascontiguousarray(tokens, np.uint32)
    out = np.zeros(t.size, f32)
    probe().lp_logprobs(v.ctypes.data, v.size, t.ctypes.data, t.size, out.ctypes.data)
    return out


def c_logprob(v, token):
    return c_logprobs(v, [token])[0]


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def model(v, tokens):
    """float64: v_t - logsumexp(v), and v_t - max(v)"""
    v = np.asarray(v, np.float64)
    M = v.max()
    lse = M + np.log(np.exp(v - M).sum())
    t = np.asarray(tokens)
    return v[t] - lse, v[t] - M


def patterns(n):
    """(name, vector): the rows of the issue's list. Shared with tests/test_hip_logprob.py."""
    rng = np.random.default_rng(1000 + n)
    last = (n - 1) // BLOCK * BLOCK  # the start of the last block
    alone = rng.standard_normal(n).astype(f32)
    alone[last + (n - last) // 2] = 9.0  # the maximum alone in the last (short) block
    one_block = (rng.standard_normal(n) - 100.0).astype(f32)  # all mass in one block, the others 100 below
    mass = BLOCK if n > BLOCK else 0
    one_block[mass:mass + BLOCK] += f32(100.0)
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(f32)
    return [("normal", rng.standard_normal(n).astype(f32)), ("normal_x8", (8.0 * rng.standard_normal(n)).astype(f32)),
            ("all_equal", np.full(n, -1.25, f32)), ("ramp", np.arange(n, dtype=f32) * f32(0.01)), ("max_alone_in_last_block", alone),
            ("one_block", one_block), ("signed_zeros", zeros)]


def tokens_of(v):
    """the maximum, the minimum, index 0, index n - 1, both sides of every block edge"""
    n = v.size
    t = [int(np.argmax(v)), int(np.argmin(v)), 0, n - 1]
    for e in range(BLOCK, n, BLOCK):
        t += [e - 1, e]
    return t


# ── 1. sample_log ──────────────────────────────────────────────────────────────────────────────────────────────────────

def test_sample_log_against_float64():
    lib = probe()
    xs = np.exp(np.linspace(np.log(0.5), np.log(2.0 ** 32), 200001)).astype(f32)
    pows = np.array([2.0 ** e for e in range(-1, 32)], f32)
    xs = np.concatenate([xs, pows, np.nextafter(pows, f32(np.inf)), np.nextafter(pows[1:], f32(0))])
    xs = xs[(xs >= 0.5) & (xs < 2.0 ** 32)]
    got = np.array([lib.lp_log(float(x)) for x in xs], np.float64)
    want = np.log(xs.astype(np.float64))
    err = np.abs(got - want)
    big = np.abs(want) >= 1.0
    rel, small = (err[big] / np.abs(want[big])).max(), err[~big].max()
    print(f"sample_log: max relative error {rel:.3g} where |ln x| >= 1, max absolute error {small:.3g} below")
    # one rounding of the result (6e-8 relative) and one of the polynomial's t + y (6e-8 of |t| <= 0.42): under 1.2e-7 either way
    assert rel <= 1.2e-7 and small <= 1.2e-7
    assert bits(lib.lp_log(1.0))[0] == 0  # +0


# ── 2. the vectors ─────────────────────────────────────────────────────────────────────────────────────────────────────

def bar(d):
    return 1e-5 + 2.4e-7 * np.abs(d)


@pytest.mark.parametrize("n", SIZES)
def test_header_against_float64(n):
    worst = 0.0
    for name, v in patterns(n):
        t = tokens_of(v)
        got = c_logprobs(v, t).astype(np.float64)
        want, d = model(v, t)
        err = np.abs(got - want)
        worst = max(worst, float((err - 2.4e-7 * np.abs(d)).max()))
        assert np.all(err <= bar(d)), (name, n, float((err - bar(d)).max()))
    print(f"n = {n}: max of |error| - 2.4e-7 |v_t - M| = {worst:.3g}")


# ── 3. edges, sums, order ──────────────────────────────────────────────────────────────────────────────────────────────

def test_edges_by_bits():
    ninf, nan = f32(-np.inf), f32(np.nan)
    v = np.array([0.5, ninf, nan, -2.0], f32)
    got = c_logprobs(v, [0, 1, 2, 3])
    assert bits(got)[1] == NEG_INF_WORD and bits(got)[2] == NEG_INF_WORD  # v_t = -inf or NaN under a finite M
    want, _ = model(np.array([0.5, -2.0]), [0, 1])
    assert abs(got[0] - want[0]) < 1e-6 and abs(got[3] - want[1]) < 1e-6  # the NaN and the -inf carry no mass
    for n in (1, 3, 5000):  # no entry above -inf: -inf for every token
        for fill in (ninf, nan):
            assert bits(c_logprobs(np.full(n, fill, f32), [0, n - 1])).tolist() == [NEG_INF_WORD] * 2
    for n in (1, 3, 5000):  # M = +inf: the quiet NaN for every token
        v = np.zeros(n, f32)
        v[n // 2] = np.inf
        assert bits(c_logprobs(v, [0, n // 2, n - 1])).tolist() == [NAN_WORD] * 3
    for x in (0.0, -0.0, 3.5, -1e30, 1e30):  # n = 1 with a finite logit: +0.0f
        assert bits(c_logprob(np.array([x], f32), 0)) == 0


def test_probabilities_sum_to_one():
    n = 1000
    for name, v in patterns(n):
        p = np.exp(c_logprobs(v, np.arange(n)).astype(np.float64)).sum()
        assert abs(p - 1.0) <= n * 1e-6, (name, p)


def test_block_independence_by_bits():
    """accumulator j of a block sums the block's elements j, j + 1024, j + 2048, j + 3072, ascending. With the other two terms 0,
    swapping the remaining two (x + y == y + x) or moving one into an empty slot of the same accumulator changes no bit."""
    rng = np.random.default_rng(7)
    n = 3 * BLOCK + 100
    v = rng.standard_normal(n).astype(f32)
    tok = [0, 5000, n - 1]
    for j, blk in ((17, 1), (1023, 0), (500, 2)):
        a, b = blk * BLOCK + j, blk * BLOCK + j + 2048
        w = v.copy()
        w[[blk * BLOCK + j + 1024, blk * BLOCK + j + 3072]] = -np.inf  # the accumulator's other two terms: 0
        base = bits(c_logprobs(w, tok))
        w[[a, b]] = w[[b, a]]  # x + y == y + x
        assert np.array_equal(bits(c_logprobs(w, tok)), base)
    # ... and a value moved to a slot of the same accumulator that held nothing
    w = v.copy()
    w[[BLOCK + 17 + 1024, BLOCK + 17 + 2048, BLOCK + 17 + 3072]] = -np.inf
    base = bits(c_logprobs(w, tok))
    w[BLOCK + 17 + 2048], w[BLOCK + 17] = w[BLOCK + 17], f32(-np.inf)
    assert np.array_equal(bits(c_logprobs(w, tok)), base)
    m, s = np.zeros(4, f32), np.zeros(4, f32)
    assert probe().lp_partials(v.ctypes.data, n, m.ctypes.data, s.ctypes.data) == 4
    assert np.array_equal(m, [v[b * BLOCK:(b + 1) * BLOCK].max() for b in range(4)])  # the block maxima are exact


def test_permutation_across_blocks_stays_within_the_bar():
    rng = np.random.default_rng(11)
    n = 50001
    v = (4.0 * rng.standard_normal(n)).astype(f32)
    perm = rng.permutation(n)
    t = np.array(tokens_of(v))
    a = c_logprobs(v, t).astype(np.float64)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    b = c_logprobs(v[perm], inv[t]).astype(np.float64)  # the same tokens at their new places
    want, d = model(v, t)
    assert np.all(np.abs(a - want) <= bar(d)) and np.all(np.abs(b - want) <= bar(d))


# ── 4. the refusals and the boundary ───────────────────────────────────────────────────────────────────────────────────

def test_refusals():
    lib = probe()
    tok, out = np.array([0, 5, 9], np.uint32), np.zeros(3, f32)

    def check(buf, off, n, rows, t=tok, o=out):
        return lib.lp_check(buf, off, n, rows, t.ctypes.data if t is not None else None, o.ctypes.data if o is not None else None)

    assert check(100, 0, 10, 3) is None and check(100, 70, 10, 3) is None and check(1 << 21, 0, 1 << 20, 1) is None
    assert b"1 .. 2^20" in check(100, 0, 0, 3) and b"1 .. 2^20" in check(1 << 22, 0, (1 << 20) + 1, 1)
    assert b"rows" in check(100, 0, 10, 0)
    assert b"inside the buffer" in check(100, 71, 10, 3) and b"inside the buffer" in check(100, 101, 10, 1) and b"inside the buffer" in check(0, 0, 10, 1)
    assert b"token out of range" in check(100, 0, 9, 3) and b"token out of range" in check(100, 0, 5, 2)
    assert b"NULL" in check(100, 0, 10, 3, t=None) and b"NULL" in check(100, 0, 10, 3, o=None)
    assert lib.lp_field_check(1, 1 << 20) is None and lib.lp_field_check(0, 1 << 30) is None
    assert b"2^20" in lib.lp_field_check(1, (1 << 20) + 1)


def test_word_takes_the_padding_and_is_off_by_default(tmp_path):
    """`logprobs` is the four bytes that were padding between `stream` and `seed`: no other field moves, the size stays"""
    fields = [n for n, _ in capi.SamplingC._fields_]
    at = fields.index("logprobs")
    assert fields[at - 1] == "stream" and fields[at + 1] == "seed"
    body = 'printf("%zu %zu %zu %zu\\n", sizeof(zgml_sampling), offsetof(zgml_sampling, stream), offsetof(zgml_sampling, logprobs), offsetof(zgml_sampling, seed));'
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.SamplingC), capi.SamplingC.stream.offset, capi.SamplingC.logprobs.offset, capi.SamplingC.seed.offset] == [80, 32, 36, 40]
    assert capi.SamplingC.of(0.8, 40, 0.95, seed=1).logprobs == 0
    sp = capi.SamplingC.of(0.8, 40, 0.95, seed=1, recent=[1, 2], penalty_window=4, repeat_penalty=1.1)
    on = capi.with_logprobs(sp)
    assert (sp.logprobs, on.logprobs) == (0, 1) and on.n_recent == 2 and on.recent[1] == 2 and capi.SamplingC.of(logprobs=True).logprobs == 1
    lib = capi.load_hip()
    for name in ("zgml_hip_logprobs", "zgml_hip_logprobs_result"):
        assert name in capi.HIP_SYMBOLS and hasattr(lib, name)


# ── 5. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "logprob_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DLOGPROB_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "logprob_probe ok" in r.stdout, r.stdout + r.stderr
