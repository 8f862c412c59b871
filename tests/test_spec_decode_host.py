"""CPU tests of greedy-exact speculative decode (include/zgml_hip.h: zgml_hip_resident_decode_speculative).

1. The draft and acceptance rules of zgml_amd/csrc/spec.h — the functions the kernels call — through the shim
   tests/cpp/spec_probe.cpp (g++), against the Python model tests/spec_model.py on random histories over small alphabets.
2. The algorithm end to end on the oracle: the model's loop over a token_len = T session, every verify step one execution of the
   T-plan, reproduces the sequential greedy decode of the token_len = 1 plan — whatever the drafts are. Rejected candidates leave
   KV columns behind; the run shows they are always overwritten before they are read.
3. The entry point is exported and declared in the ctypes mirror."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "cpp" / "_build" / "libspec_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "spec_probe.cpp", ROOT / "zgml_amd" / "csrc" / "spec.h"]
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u32 = C.c_void_p, C.c_uint32
    lib.sp_candidates_lookup.argtypes, lib.sp_candidates_lookup.restype = [vp, u32, u32, u32, vp, vp], u32
    lib.sp_ngram_find.argtypes, lib.sp_ngram_find.restype = [vp, u32, u32], C.c_int64
    lib.sp_candidates_provided.argtypes, lib.sp_candidates_provided.restype = [u32, u32, u32, vp, u32, u32, vp], u32
    lib.sp_accept.argtypes, lib.sp_accept.restype = [vp, vp, u32], u32
    lib.sp_emit_count.argtypes, lib.sp_emit_count.restype = [u32, u32, u32], u32
    _lib = lib
    return lib


def c_lookup(hist, pos, ngram, T):
    h = np.ascontiguousarray(hist, np.uint32)
    cand, match = np.full(T, 0xFFFFFFFF, np.uint32), C.c_int64(-7)
    real = probe().sp_candidates_lookup(h.ctypes.data, pos, ngram, T, cand.ctypes.data, C.byref(match))
    return cand.tolist(), int(real), (None if match.value < 0 else int(match.value))


# ── 1. spec.h against the model ────────────────────────────────────────────────────────────────────────────────────────

def test_lookup_drafts_match_the_model_on_random_histories():
    rng = np.random.default_rng(20)
    seen = {"no_match": 0, "periodic": 0, "short": 0, "match": 0}
    for case in range(600):
        alphabet = int(rng.integers(2, 6))
        length = int(rng.integers(1, 41))
        T, ngram = int(rng.integers(2, 7)), int(rng.integers(1, 5))
        hist = rng.integers(0, alphabet, length).tolist()
        pos = length - 1
        want_c, want_real = SM.candidates_lookup(hist, pos, T, ngram)
        want_i = SM.lookup(hist, pos, ngram)
        got_c, got_real, got_i = c_lookup(hist + [99] * T, pos, ngram, T)  # (the words behind hist[pos] must not be read: 99 is in no alphabet)
        assert (got_c, got_real, got_i) == (want_c, want_real, want_i), (hist, T, ngram)
        assert 99 not in got_c
        seen["no_match"] += want_i is None
        seen["match"] += want_i is not None
        seen["periodic"] += want_i == pos - 1
        seen["short"] += pos < ngram
    assert all(v >= 10 for v in seen.values()), seen  # every kind of case occurred


def test_lookup_cases_by_hand():
    # the longest suffix wins over a later occurrence of a shorter one: "1 2" occurred at 1..2, "2" alone also at 5
    assert c_lookup([0, 1, 2, 3, 4, 2, 7, 1, 2], 8, 2, 4) == ([2, 3, 4, 2], 3, 2)
    assert c_lookup([0, 1, 2, 3, 4, 2, 7, 1, 2], 8, 1, 4) == ([2, 7, 1, 2], 3, 5)
    # a match at pos - 1 continues periodically through its own drafts
    assert c_lookup([5, 5], 1, 2, 5) == ([5, 5, 5, 5, 5], 4, 0)  # (n = 2 does not apply at pos 1; n = 1 matches at 0)
    assert c_lookup([3, 1, 2, 1, 2], 4, 2, 6) == ([2, 1, 2, 1, 2, 1], 5, 2)
    # no match at any n: every candidate is a pad, nothing is drafted
    assert c_lookup([4, 3, 2, 1], 3, 4, 3) == ([1, 1, 1], 0, None)
    assert c_lookup([6], 0, 4, 2) == ([6, 6], 0, None)
    # one suffix length alone: the largest i, and lengths that do not apply
    h = np.array([1, 1, 1, 1], np.uint32)
    assert [probe().sp_ngram_find(h.ctypes.data, 3, n) for n in (1, 2, 3, 4, 5)] == [2, 2, 2, -1, -1]


def test_provided_drafts_and_acceptance_match_the_model():
    rng = np.random.default_rng(21)
    lib = probe()
    for case in range(400):
        T = int(rng.integers(2, 7))
        start = int(rng.integers(0, 9))
        pos = start + int(rng.integers(0, 12))
        drafts = rng.integers(0, 5, int(rng.integers(0, 16))).astype(np.uint32)
        tok = int(rng.integers(0, 5))
        cand = np.zeros(T, np.uint32)
        d_ptr = drafts.ctypes.data if drafts.size else None
        real = lib.sp_candidates_provided(tok, pos, start, d_ptr, drafts.size, T, cand.ctypes.data)
        assert (cand.tolist(), real) == SM.candidates_provided(tok, pos, start, drafts, T)
        g = rng.integers(0, 3, T).astype(np.uint32)
        c2 = rng.integers(0, 3, T).astype(np.uint32)
        a = lib.sp_accept(c2.ctypes.data, g.ctypes.data, T)
        assert a == SM.accept(c2.tolist(), g.tolist()) and 0 <= a <= T - 1
        n_tokens, produced = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        assert lib.sp_emit_count(a, n_tokens, produced) == max(0, min(a + 1, n_tokens - produced))
    # a pad that happens to be the greedy token is accepted like any other candidate
    c, g = np.array([7, 7, 7], np.uint32), np.array([7, 7, 2], np.uint32)
    assert lib.sp_accept(c.ctypes.data, g.ctypes.data, 3) == 2


# ── 2. the algorithm on the oracle ─────────────────────────────────────────────────────────────────────────────────────

N, START_TOKEN = 24, 3
T_MAX = 5


@pytest.fixture(scope="module")
def tiny_stream(oracle):
    """the oracle's sequential greedy decode of the token_len = 1 plan: N + T_MAX tokens from START_TOKEN at position 0"""
    cfg = llama.preset("tiny", 64)
    m = llama.Model(cfg, llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    tok, out = START_TOKEN, []
    for pos in range(N + T_MAX):
        tok, _ = s.step(tok, pos)
        out.append(tok)
    s.close(), m.close()
    return out


def oracle_rows(oracle, T):
    """rows_fn of the model's loop: one execution of the token_len = T plan on the oracle, all T logits rows read from its buffer"""
    cfg = llama.preset("tiny", 64)
    m = llama.Model(cfg, llama.Q4_0, token_len=T)
    s = llama.Session(m, oracle.backend_fns())
    ob = oracle.OracleBackend()

    def rows(c, pos):
        s.prefill(c, pos, want_logits=False)
        logits = ob.buffer(s.handle, m.buf("logits"))[:T * cfg.vocab_size].reshape(T, cfg.vocab_size)
        return [oracle.argmax(logits[j]) for j in range(T)]
    return rows, (s, m)


def wrong_at(stream, vocab, where):
    d = [int(t) for t in stream]
    for i in where:
        d[i] = (d[i] + 1) % vocab
    return d


DRAFT_FORMS = ["perfect", "wrong_everywhere", "wrong_at_two", "ngram"]


def drafts_of(form, stream, vocab):
    """provided drafts (drafts[i] = guess for the token at position start + 1 + i, i.e. for stream[i]) of a named form; None = n-gram"""
    if form == "perfect":
        return [int(t) for t in stream]
    if form == "wrong_everywhere":
        return wrong_at(stream, vocab, range(len(stream)))
    if form == "wrong_at_two":
        return wrong_at(stream, vocab, (5, 14))
    return None


@pytest.mark.parametrize("T", [2, 4, 5])
def test_model_loop_on_the_oracle_reproduces_sequential_greedy_decode(oracle, tiny_stream, T):
    vocab = llama.preset("tiny", 64).vocab_size
    rows, keep = oracle_rows(oracle, T)
    for form in DRAFT_FORMS:
        drafts = drafts_of(form, tiny_stream, vocab)
        toks, stats = SM.spec_loop(rows, START_TOKEN, 0, N, T, drafts=drafts)
        assert toks == tiny_stream[:N], form
        assert stats == SM.predict(tiny_stream, START_TOKEN, 0, N, T, drafts=drafts), form  # what the GPU tests will expect
        if form == "perfect":
            assert stats == {"steps": -(-N // T), "drafted": (T - 1) * -(-N // T), "accepted": (T - 1) * -(-N // T)}
        if form == "wrong_everywhere":
            assert stats == {"steps": N, "drafted": (T - 1) * N, "accepted": 0}
        if form == "wrong_at_two":
            assert -(-N // T) < stats["steps"] < N
    keep[0].close(), keep[1].close()


# ── 3. the ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_entry_point_is_exported_and_mirrored(tmp_path):
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    assert "zgml_hip_resident_decode_speculative" in capi.HIP_SYMBOLS and hasattr(lib, "zgml_hip_resident_decode_speculative")
    # the two records as gcc lays them out against the ctypes mirror
    fields = ["history", "n_history", "mode", "drafts", "n_drafts", "ngram"]
    body = 'printf("%zu %zu ", sizeof(zgml_spec_decode), sizeof(zgml_spec_stats));'
    body += "".join(f'printf("%zu ", offsetof(zgml_spec_decode, {f}));' for f in fields)
    body += 'printf("%zu", offsetof(zgml_spec_stats, accepted));'
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "zgml_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(capi.SpecDecodeC), C.sizeof(capi.SpecStatsC)] + [getattr(capi.SpecDecodeC, f).offset for f in fields] + [capi.SpecStatsC.accepted.offset]
    assert got == want
    assert hasattr(llama.Session, "resident_decode_speculative")
