"""CPU tests of the rule of the alternatives (include/zgml_hip.h: the `top_logprobs` word of zgml_sampling, zgml_hip_top_logprobs).
The rule is zgml_amd/csrc/sample.h ("THE ALTERNATIVES") — the functions the kernel of top_logprob.hip calls — reached through
tests/cpp/top_logprob_probe.cpp (g++ -ffp-contract=off):

1. The rule against float64 numpy: the tokens are the order "value descending, index ascending" exactly (v + 0.0: signed zeros
   tie); the values lie within the bar of tests/test_logprob_host.py, 1e-5 + 2.4e-7 |v_t - M| (the values ARE that rule's, so its
   derivation holds unchanged).
2. Bit identities: value_j is the log-probability probe's value of token_j; entry 0 is the first maximum; without penalties the
   tokens are the sample probe's first candidates.
3. The sliced form equals the direct form, by bits.
4. The edges, by bits.
5. The host logic of zgml_amd/csrc/sample_params.h; the word's place in zgml_sampling.
6. The probe's stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi
from tests.test_logprob_host import NAN_WORD, NEG_INF_WORD, bar, bits, c_logprobs, patterns
from tests.test_sample_host import c_candidates

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libtop_logprob_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "top_logprob_probe.cpp", ROOT / "zgml_amd" / "csrc" / "sample.h", ROOT / "zgml_amd" / "csrc" / "sample_params.h",
        ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
f32 = np.float32
TOP_MAX = 64
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1792, 1793, 4096, 4097, 8193, 50001, 57345]
COUNTS = [1, 5, 64]
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", *FLAGS, "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.tl_top.argtypes, lib.tl_top.restype = [vp, u64, u32, u32, vp, vp, u32], u32
    lib.tl_count.argtypes, lib.tl_count.restype = [u32, u64], u32
    lib.tl_slices.argtypes, lib.tl_slices.restype = [u64], u32
    lib.tl_slice_len.argtypes, lib.tl_slice_len.restype = [u64], u32
    lib.tl_check.argtypes, lib.tl_check.restype = [u64, u64, u64, u32, u32, vp, vp], C.c_char_p
    lib.tl_word.argtypes, lib.tl_word.restype = [u32, u32], u32
    _lib = lib
    return lib


def c_top(v, a, width=None, sliced=False):
    """the header's alternatives of the row v for the count a: (tokens int64[width], values float32[width]), -1 / NaN behind a_eff
    (what the device's must equal, to the bit). width: a by default. sliced: False the direct form, True the sliced form as the
    select launch cuts the row, an int > 1 the sliced form over slices of that many logits"""
    v = np.ascontiguousarray(v, f32)
    width = a if width is None else width
    tok, val = np.zeros(width, np.int64), np.zeros(width, f32)
    assert probe().tl_top(v.ctypes.data, v.size, a, width, tok.ctypes.data, val.ctypes.data, int(sliced)) == min(a, TOP_MAX, v.size)
    return tok, val


def slice_bounds(n):
    """[(lo, hi)] of the non-empty slices of a row of n logits"""
    lib = probe()
    slices, ln = lib.tl_slices(n), lib.tl_slice_len(n)
    return [(l * ln, min(l * ln + ln, n)) for l in range(slices) if l * ln < n]


def planted(n):
    """64 large distinct values, two in each of the (up to 32) slices, at the slice's first and last index, over small noise"""
    rng = np.random.default_rng(2000 + n)
    v = (0.1 * rng.standard_normal(n)).astype(f32)
    vals = rng.permutation(64).astype(f32) * f32(0.25) + f32(10.0)
    for l, (lo, hi) in enumerate(slice_bounds(n)):
        v[lo] = vals[2 * l]
        v[hi - 1] = vals[2 * l + 1]  # (a slice of one element: the second value stands)
    return v


def rows_of(n):
    """the rows of the issue's list: the patterns of tests/test_logprob_host.py and the planted row. Shared with
    tests/test_hip_top_logprob.py."""
    return patterns(n) + [("planted", planted(n))]


def edge_rows(n):
    rng = np.random.default_rng(3000 + n)
    mixed = rng.standard_normal(n).astype(f32)
    mixed[::3] = np.nan
    mixed[1::5] = -np.inf
    inf = np.zeros(n, f32)
    inf[n // 2] = np.inf
    return [("nan_and_minus_inf", mixed), ("all_minus_inf", np.full(n, -np.inf, f32)), ("holds_plus_inf", inf)]


def order(v):
    """value descending, index ascending; -0 == +0, a NaN as -inf"""
    x = np.asarray(v, np.float64) + 0.0
    x = np.where(np.isnan(x), -np.inf, x)
    return np.lexsort((np.arange(x.size), -x))


# ── 1. the rule against float64 ────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", SIZES)
def test_rule_against_float64(n):
    worst = 0.0
    for name, v in rows_of(n):
        want_order = order(v)
        v64 = v.astype(np.float64)
        M = v64.max()
        lse = M + np.log(np.exp(v64 - M).sum())
        for a in COUNTS:
            ae = min(a, n)
            tok, val = c_top(v, a)
            assert probe().tl_count(a, n) == ae
            assert tok[:ae].tolist() == want_order[:ae].tolist(), (name, n, a)
            assert np.all(tok[ae:] == -1) and np.all(bits(val[ae:]) == NAN_WORD)
            d = v64[tok[:ae]] - M
            err = np.abs(val[:ae].astype(np.float64) - (v64[tok[:ae]] - lse))
            worst = max(worst, float((err - 2.4e-7 * np.abs(d)).max()))
            assert np.all(err <= bar(d)), (name, n, a, float((err - bar(d)).max()))
    print(f"n = {n}: max of |error| - 2.4e-7 |v_t - M| = {worst:.3g}")


# ── 2. bit identities ──────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [1, 65, 257, 4097, 50001])
def test_bit_identities(n):
    for name, v in rows_of(n):
        tok, val = c_top(v, 64)
        ae = min(64, n)
        assert np.array_equal(bits(val[:ae]), bits(c_logprobs(v, tok[:ae]))), (name, n)  # what zgml_hip_logprobs returns for token_j
        assert tok[0] == int(np.argmax(v.astype(np.float64) + 0.0)), (name, n)  # the first maximum
        for a in COUNTS:  # penalties off, top_k >= a: the first candidates of the pick
            assert c_top(v, a)[0][:min(a, n)].tolist() == c_candidates(v, max(a, 40))[:min(a, n)], (name, n, a)


# ── 3. sliced == direct ────────────────────────────────────────────────────────────────────────────────────────────────

def sliced_rows():
    out = []
    for n in SIZES:
        out += [(n, name, v) for name, v in rows_of(n) + edge_rows(n)]
    return out


def test_a_last_slice_of_one_element():
    """The select launch cuts a row into sample_slices(n) slices of ceil(n / slices) logits, which leaves the last slice at least
    ceil(n / slices) - 31 long: with slices of 1792 and more it never holds one element alone (57345 = 32 x 1793 - 31 has the
    shortest, 1762). The merge must not depend on where the cuts are, so the one-element case is run through the sliced form with
    cuts of its own: n = 31 x len + 1."""
    assert min(hi - lo for n in range(1793, 70000, 97) for lo, hi in slice_bounds(n)[-1:]) > 1
    assert slice_bounds(57345)[-1] == (31 * 1793, 57345)
    for ln in (2, 64, 65, 1793):
        n = 31 * ln + 1
        for name, v in rows_of(n) + edge_rows(n):
            if name == "planted":
                v = v.copy()
                v[n - 1] = 99.0  # the row's maximum alone in the last slice
            for a in COUNTS:
                t0, x0 = c_top(v, a, TOP_MAX)
                t1, x1 = c_top(v, a, TOP_MAX, sliced=ln)
                assert np.array_equal(t0, t1) and np.array_equal(bits(x0), bits(x1)), (name, n, a)


def test_sliced_form_equals_direct_form_by_bits():
    for n, name, v in sliced_rows():
        for a in COUNTS + [65]:
            t0, x0 = c_top(v, a, TOP_MAX)
            t1, x1 = c_top(v, a, TOP_MAX, sliced=True)
            assert np.array_equal(t0, t1) and np.array_equal(bits(x0), bits(x1)), (name, n, a)
    n = 57345  # where the 64 come from
    bounds = slice_bounds(n)
    rows = dict(rows_of(n))
    assert c_top(rows["all_equal"], 64)[0].tolist() == list(range(64)) and bounds[0][1] >= 64  # all from slice 0
    assert c_top(rows["ramp"], 64)[0].min() >= bounds[-1][0] and len(bounds) == 32  # all from the last slice
    edges = sorted(e for lo, hi in bounds for e in (lo, hi - 1))
    assert sorted(c_top(rows["planted"], 64)[0].tolist()) == edges  # two from every slice


# ── 4. edges ───────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_edges_by_bits():
    for n in (1, 3, 70, 5000):
        rows = dict(edge_rows(n))
        for sliced in (False, True):
            tok, val = c_top(rows["all_minus_inf"], 64, sliced=sliced)
            ae = min(64, n)
            assert tok[:ae].tolist() == list(range(ae)) and np.all(bits(val[:ae]) == NEG_INF_WORD)  # tokens 0.., values -inf
            tok, val = c_top(rows["holds_plus_inf"], 64, sliced=sliced)
            assert tok[0] == n // 2 and tok[:ae].tolist() == order(rows["holds_plus_inf"])[:ae].tolist() and np.all(bits(val) == NAN_WORD)
            v = rows["nan_and_minus_inf"]
            tok, val = c_top(v, 64, sliced=sliced)
            assert tok[:ae].tolist() == order(v)[:ae].tolist()
            assert np.array_equal(bits(val[:ae]), bits(c_logprobs(v, tok[:ae])))
            dead = np.isnan(v[tok[:ae]]) | np.isinf(v[tok[:ae]])
            if n > 1:
                assert np.all(bits(val[:ae])[dead] == NEG_INF_WORD) and np.all(np.isfinite(val[:ae][~dead]))
    # n < a: -1 / NaN padding
    tok, val = c_top(np.array([0.5, 2.0, -1.0], f32), 5)
    assert tok.tolist() == [1, 0, 2, -1, -1] and bits(val[3:]).tolist() == [NAN_WORD] * 2 and np.all(val[:3] < 0)
    # n = 1: its token at +0.0f
    for x in (0.0, -0.0, 3.5, -1e30):
        tok, val = c_top(np.array([x], f32), 64)
        assert tok[0] == 0 and bits(val)[0] == 0 and np.all(tok[1:] == -1) and np.all(bits(val[1:]) == NAN_WORD)
    # signed zeros tie: the lower index first
    assert c_top(np.array([-0.0, 0.0, -0.0, 0.0], f32), 4)[0].tolist() == [0, 1, 2, 3]


# ── 5. host logic ──────────────────────────────────────────────────────────────────────────────────────────────────────

def test_refusals_of_top_logprobs():
    lib = probe()
    tok, out = np.zeros(3 * 64, np.int64), np.zeros(3 * 64, f32)

    def check(buf, off, n, rows, top_n, t=tok, o=out):
        return lib.tl_check(buf, off, n, rows, top_n, t.ctypes.data if t is not None else None, o.ctypes.data if o is not None else None)

    assert check(100, 0, 10, 3, 5) is None and check(100, 70, 10, 3, 64) is None and check(1 << 21, 0, 1 << 20, 1, 1) is None
    assert check(100, 0, 3, 3, 64) is None  # top_n above n is served (padding), not refused
    assert b"1 .. 2^20" in check(100, 0, 0, 3, 5) and b"1 .. 2^20" in check(1 << 22, 0, (1 << 20) + 1, 1, 5)
    assert b"rows" in check(100, 0, 10, 0, 5)
    assert b"inside the buffer" in check(100, 71, 10, 3, 5) and b"inside the buffer" in check(100, 101, 10, 1, 5) and b"inside the buffer" in check(0, 0, 10, 1, 5)
    assert b"NULL" in check(100, 0, 10, 3, 5, t=None) and b"NULL" in check(100, 0, 10, 3, 5, o=None)
    assert b"top_n" in check(100, 0, 10, 3, 0) and b"top_n" in check(100, 0, 10, 3, 65) and b"top_n" in check(100, 0, 10, 3, 0xFFFFFFFF)


def test_the_word_is_clamped_and_needs_logprobs():
    lib = probe()
    assert [lib.tl_word(1, a) for a in (0, 1, 5, 64, 65, 0xFFFFFFFF)] == [0, 1, 5, 64, 64, 64]  # clamped, never refused
    assert [lib.tl_word(0, a) for a in (0, 7, 0xFFFFFFFF)] == [0, 0, 0]  # ignored when logprobs == 0
    assert lib.tl_word(0xDEADBEEF, 7) == 7


def test_word_takes_the_trailing_padding_and_is_off_by_default(tmp_path):
    """`top_logprobs` is the four bytes that were padding behind `n_recent`: no field moves, the size stays. (The ctypes mirror
    reaches the word in place: padding has no name in _fields_.)"""
    assert capi.SamplingC._fields_[-1][0] == "n_recent" and capi.SamplingC.top_logprobs.size == 4
    body = 'printf("%zu %zu %zu\\n", sizeof(zgml_sampling), offsetof(zgml_sampling, n_recent), offsetof(zgml_sampling, top_logprobs));'
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.SamplingC), capi.SamplingC.n_recent.offset, capi.SamplingC.top_logprobs.offset] == [80, 72, 76]
    assert capi.SamplingC.of(0.8, 40, 0.95, seed=1).top_logprobs == 0 and capi.SamplingC.of(0.8, 40, 0.95, seed=1, logprobs=True).top_logprobs == 0
    sp = capi.SamplingC.of(0.8, 40, 0.95, seed=1, recent=[1, 2], penalty_window=4, repeat_penalty=1.1)
    on = capi.with_logprobs(sp, top=5)
    assert (sp.logprobs, sp.top_logprobs, on.logprobs, on.top_logprobs) == (0, 0, 1, 5) and on.n_recent == 2 and on.recent[1] == 2
    assert capi.with_logprobs(sp).top_logprobs == 0
    both = capi.SamplingC.of(top_logprobs=7)
    assert (both.logprobs, both.top_logprobs) == (1, 7)  # the count alone asks for the values too: the word is read only with them
    lib = capi.load_hip()
    for name in ("zgml_hip_top_logprobs", "zgml_hip_top_logprobs_result"):
        assert name in capi.HIP_SYMBOLS and hasattr(lib, name)


# ── 6. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "top_logprob_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTOP_LOGPROB_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "top_logprob_probe ok" in r.stdout, r.stdout + r.stderr
