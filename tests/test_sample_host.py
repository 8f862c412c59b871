"""CPU tests of seeded top-k / top-p sampling (include/zgml_hip.h: zgml_sampling, zgml_hip_sample, zgml_hip_resident_decode_sampled,
_batch_sampled). The rule is zgml_amd/csrc/sample.h — the functions the kernels call — reached through tests/cpp/sample_probe.cpp
(g++ -ffp-contract=off):

1. Philox4x32-10 against the Random123 known answers, and the mapping of its first word to u.
2. The candidate order against numpy.lexsort, ties, NaN, infinities and signed zeros included; top_k = 1 is the oracle's argmax.
3. The pick against the float64 model tests/sample_model.py on 3600 random cases. The model may set a case aside only under its
   two written conditions, and at most 2 % of the cases — asserted from the model alone, before the header is asked.
4. The probe's stand-alone program under AddressSanitizer + UBSan.
5. sizeof / offsets of zgml_sampling against the ctypes mirror; the entry points are exported."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi
from tests import sample_model as M

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libsample_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "sample_probe.cpp", ROOT / "zgml_amd" / "csrc" / "sample.h"]
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib.sp_philox.argtypes, lib.sp_philox.restype = [vp, vp, vp], None
    lib.sp_u_of_word.argtypes, lib.sp_u_of_word.restype = [u32], f32
    lib.sp_uniform.argtypes, lib.sp_uniform.restype = [u64, u32, u32], f32
    lib.sp_exp.argtypes, lib.sp_exp.restype = [f32], f32
    lib.sp_candidates.argtypes, lib.sp_candidates.restype = [vp, u32, u32, vp], u32
    lib.sp_pick.argtypes, lib.sp_pick.restype = [vp, u32, u32, f32, f32, f32, C.POINTER(u32)], u32
    lib.sp_sample.argtypes, lib.sp_sample.restype = [vp, u32, u32, f32, f32, u64, u32, u32], u32
    _lib = lib
    return lib


def c_candidates(v, top_k):
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros(256, np.uint32)
    k = probe().sp_candidates(v.ctypes.data, v.size, top_k, out.ctypes.data)
    return out[:k].tolist()


def c_sample(v, sp, position):
    """the header's token for logits v under the capi.SamplingC sp at `position` (what a device pick must equal)"""
    v = np.ascontiguousarray(v, np.float32)
    return int(probe().sp_sample(v.ctypes.data, v.size, sp.top_k, sp.temperature, sp.top_p, sp.seed, sp.stream, position))


# ── 1. the random number ───────────────────────────────────────────────────────────────────────────────────────────────

def philox(ctr, key):
    c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    probe().sp_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return [int(x) for x in out]


def test_philox_known_answers():
    assert philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_u_mapping():
    lib = probe()
    assert lib.sp_u_of_word(0xFFFFFFFF) == 1.0 - 2.0 ** -24
    assert lib.sp_u_of_word(0) == 0.0 and lib.sp_u_of_word(0xFF) == 0.0 and lib.sp_u_of_word(0x100) == 2.0 ** -24
    rng = np.random.default_rng(3)
    for seed, stream, pos in rng.integers(0, 2 ** 32, (200, 3)):
        seed = int(seed) | (int(stream) << 37)  # (both key words in use)
        u = lib.sp_uniform(seed, int(stream), int(pos))
        assert 0.0 <= u < 1.0
        # counter (position, stream, 0, 0), key (seed low, seed high), the first word
        w0 = philox([int(pos), int(stream), 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])[0]
        assert u == (w0 >> 8) * 2.0 ** -24


def test_sample_exp_is_accurate_and_never_denormal():
    lib = probe()
    x = np.concatenate([np.linspace(-80, 0, 20001), -np.logspace(-8, 1.9, 4000)]).astype(np.float32)
    got = np.array([lib.sp_exp(float(a)) for a in x], np.float64)
    # the Taylor remainder (ln 2 / 2)^7 / 5040 over the smallest e^r = 2^-1/2 is 1.7e-7; a few f32 roundings of the Horner steps on top
    assert np.max(np.abs(got / np.exp(x.astype(np.float64)) - 1)) <= 3e-7
    assert lib.sp_exp(0.0) == 1.0
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert lib.sp_exp(-87.0) >= tiny
    for a in (-87.0001, -88.0, -1000.0, float("-inf"), float("nan")):
        assert lib.sp_exp(a) == 0.0


# ── 2. the candidate order ─────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("top_k", [0, 1, 2, 40, 256])
def test_candidates_match_lexsort(top_k):
    rng = np.random.default_rng(top_k)
    for n in (1, 2, 39, 255, 256, 257, 1000, 4097):
        vs = [rng.standard_normal(n), np.round(rng.standard_normal(n) * 2) / 2, np.full(n, 1.5), np.zeros(n)]
        mixed = rng.standard_normal(n)  # a sixth of the entries each: NaN, +inf, -inf, +0, -0, a finite value
        kind = rng.integers(0, 6, n)
        for code, val in enumerate([np.nan, np.inf, -np.inf, 0.0, -0.0]):
            mixed[kind == code] = val
        for v in vs + [mixed]:
            v = v.astype(np.float32)
            assert c_candidates(v, top_k) == M.candidates(v, top_k).tolist(), (n, top_k)


def test_all_equal_gives_the_lowest_indices():
    assert c_candidates(np.full(1000, -3.25, np.float32), 40) == list(range(40))
    assert c_candidates(np.array([0.0, -0.0] * 300, np.float32), 0) == list(range(256))
    assert c_candidates(np.full(5, np.nan, np.float32), 256) == list(range(5))  # (n < top_k; NaN == -inf)


def test_top_k_1_is_the_argmax(oracle):
    rng = np.random.default_rng(11)
    for n in (1, 7, 256, 3000):
        for v in (rng.standard_normal(n), np.round(rng.standard_normal(n)), np.where(rng.random(n) < 0.5, 0.0, -0.0)):
            v = v.astype(np.float32)
            assert c_candidates(v, 1) == [oracle.argmax(v)]
            sp = capi.SamplingC.of(temperature=0.7, top_k=1, seed=5)
            assert c_sample(v, sp, 3) == oracle.argmax(v)


# ── 3. the pick against the float64 model ──────────────────────────────────────────────────────────────────────────────

def pick_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for k in (1, 2, 5, 40, 64, 256):
        for T in (0.25, 0.7, 1.0, 1.5, 4.0):
            for top_p in (0.5, 0.9, 0.95, 1.0):
                for spread in (0.5, 4.0, 20.0):
                    for _ in range(10):
                        v = (rng.standard_normal(300) * spread).astype(np.float32)
                        if rng.random() < 0.3:
                            v = (np.round(v * 4) / 4).astype(np.float32)  # ties
                        u = float(rng.integers(0, 1 << 24)) * 2.0 ** -24
                        cases.append((v, k, T, top_p, u))
    return cases


def test_pick_matches_the_float64_model():
    cases = pick_cases()
    assert len(cases) >= 3000
    want = []
    for v, k, T, top_p, u in cases:
        cand = M.candidates(v, k)
        rank, ambiguous = M.pick(v[cand], T, top_p, u)
        want.append((int(cand[rank]), rank, ambiguous))
    set_aside = sum(a for _, _, a in want)
    print(f"set aside as ambiguous: {set_aside} of {len(cases)}")
    assert set_aside <= 0.02 * len(cases)  # a condition on the cases, checked before the header is asked
    lib, wrong, wrong_without_margin = probe(), [], 0
    for (v, k, T, top_p, u), (tok, rank, ambiguous) in zip(cases, want):
        r = C.c_uint32(0)
        got = int(lib.sp_pick(v.ctypes.data, v.size, k, T, top_p, u, C.byref(r)))
        if (got, r.value) != (tok, rank):
            wrong_without_margin += 1
            if not ambiguous:
                wrong.append((k, T, top_p, u, got, tok))
    print(f"disagreements: {len(wrong)} outside the margin, {wrong_without_margin} in all")
    assert not wrong, wrong[:5]


def test_sample_is_pick_at_the_philox_u():
    lib, rng = probe(), np.random.default_rng(8)
    v = rng.standard_normal(700).astype(np.float32)
    toks = set()
    for pos in range(64):
        u = lib.sp_uniform(77, 2, pos)
        want = int(lib.sp_pick(v.ctypes.data, v.size, 40, 0.8, 0.95, u, None))
        assert c_sample(v, capi.SamplingC.of(0.8, 40, 0.95, seed=77, stream=2), pos) == want
        toks.add(want)
    assert len(toks) > 5  # (it does sample)


def test_a_minus_inf_candidate_is_never_picked():
    v = np.full(500, -np.inf, np.float32)
    v[[17, 255, 256]] = [1.0, 0.5, 1.0]
    assert c_candidates(v, 40)[:3] == [17, 256, 255]
    for pos in range(200):
        assert c_sample(v, capi.SamplingC.of(1.5, 40, 1.0, seed=1), pos) in (17, 255, 256)


# ── 4. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "sample_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DSAMPLE_PROBE_MAIN", "-o", str(exe), str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "sample_probe ok" in r.stdout, r.stdout + r.stderr


# ── 5. the boundary ────────────────────────────────────────────────────────────────────────────────────────────────────

def test_sampling_struct_layout_matches_c(tmp_path):
    fields = [n for n, _ in capi.SamplingC._fields_]
    body = 'printf("%zu\\n", sizeof(zgml_sampling));' + "".join(f'printf("%zu\\n", offsetof(zgml_sampling, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "sz")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.SamplingC)] + [getattr(capi.SamplingC, f).offset for f in fields]


def test_entry_points_are_exported():
    lib = capi.load_hip()
    for name in ("zgml_hip_sample", "zgml_hip_resident_decode_sampled", "zgml_hip_resident_decode_batch_sampled"):
        assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
