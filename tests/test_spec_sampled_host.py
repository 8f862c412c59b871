"""CPU tests of sampled speculative decode (include/zgml_hip.h: zgml_hip_resident_decode_speculative_sampled).

1. The stop cut of zgml_amd/csrc/spec.h — the function spec_accept_kernel calls — through tests/cpp/spec_sampled_probe.cpp
   (g++ -ffp-contract=off) against the Python model tests/spec_sampled_model.py, on random cases and on the named ones.
2. The algorithm end to end on the oracle: the model's loop over a token_len = T session with every logits row sampled by the
   header's rule at its own position gives the same tokens whatever the drafts are; with top_k = 1 they are the oracle's
   sequential greedy stream; and — under the condition that the T-plan's rows and the decode plan's rows are bit-equal, asserted
   first — they are the sequential sampled decode of the token_len = 1 plan.
3. The probe's stand-alone program under AddressSanitizer + UBSan.
4. The entry point is exported and declared in the ctypes mirror."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.test_sample_host import c_sample

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libspec_sampled_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "spec_sampled_probe.cpp", ROOT / "zgml_amd" / "csrc" / "spec.h", ROOT / "zgml_amd" / "csrc" / "sample.h"]
S = capi.SamplingC.of
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
    lib.ssp_stop_cut.argtypes, lib.ssp_stop_cut.restype = [vp, u32, u32, vp, C.POINTER(C.c_int32)], u32
    lib.ssp_sample.argtypes, lib.ssp_sample.restype = [vp, u32, u32, f32, f32, u64, u32, u32], u32
    lib.ssp_step.argtypes, lib.ssp_step.restype = [vp, vp, u32, u32, u32, u32, vp, vp], None
    _lib = lib
    return lib


def c_stop_cut(g, m, stop):
    g = np.ascontiguousarray(g, np.uint32)
    st = np.ascontiguousarray(stop, np.uint32)
    fired = C.c_int32(-7)
    cut = probe().ssp_stop_cut(g.ctypes.data, m, st.size, st.ctypes.data if st.size else None, C.byref(fired))
    return int(cut), bool(fired.value)


# ── 1. the stop cut against the model ──────────────────────────────────────────────────────────────────────────────────

def test_stop_cut_cases_by_hand():
    g = [5, 6, 7, 8]
    assert c_stop_cut(g, 4, [5]) == (1, True) == SSM.stop_cut(g, 4, {5})       # a stop at g[0]
    assert c_stop_cut(g, 4, [8]) == (4, True) == SSM.stop_cut(g, 4, {8})       # a stop at g[m - 1]: fires, cuts nothing
    assert c_stop_cut(g, 2, [7]) == (2, False) == SSM.stop_cut(g, 2, {7})      # a stop behind the cut does not fire
    assert c_stop_cut(g, 3, [8]) == (3, False) == SSM.stop_cut(g, 3, {8})
    assert c_stop_cut(g, 4, []) == (4, False) == SSM.stop_cut(g, 4, set())     # n_stop = 0
    assert c_stop_cut(g, 4, [9, 7, 6, 1]) == (2, True)                         # the first stop token in g's order, not in the set's
    assert c_stop_cut([3, 3, 3], 3, [3]) == (1, True)
    assert c_stop_cut(g, 0, [5]) == (0, False)                                 # an idle step emits nothing and stops nothing


def test_stop_cut_matches_the_model_on_random_cases():
    rng = np.random.default_rng(31)
    seen = {"first": 0, "last": 0, "behind": 0, "none": 0, "inside": 0, "no_set": 0}
    for case in range(2000):
        T = int(rng.integers(2, 7))
        g = rng.integers(0, 6, T).tolist()
        m = int(rng.integers(0, T + 1))
        stop = rng.integers(0, 9, int(rng.integers(0, 5))).tolist()
        want = SSM.stop_cut(g, m, set(stop))
        assert c_stop_cut(g + [stop[0] if stop else 0], m, stop) == want, (g, m, stop)  # (the word behind g[T - 1] is not looked at either)
        seen["no_set"] += not stop
        seen["none"] += bool(stop) and not want[1]
        seen["first"] += want == (1, True) and m > 1
        seen["last"] += want == (m, True) and m > 1
        seen["inside"] += want[1] and 1 < want[0] < m
        seen["behind"] += not want[1] and any(t in stop for t in g[m:])
    assert all(v >= 20 for v in seen.values()), seen  # every kind of case occurred


def test_a_step_is_accept_then_emit_count_then_stop_cut():
    """the order spec_accept_kernel applies the rules in: `accepted` counts before any cut"""
    rng = np.random.default_rng(32)
    lib = probe()
    for case in range(600):
        T = int(rng.integers(2, 7))
        c, g = rng.integers(0, 3, T).astype(np.uint32), rng.integers(0, 3, T).astype(np.uint32)
        stop = rng.integers(0, 4, int(rng.integers(0, 5))).astype(np.uint32)
        wanted, produced = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        out = np.zeros(3, np.uint32)
        lib.ssp_step(c.ctypes.data, g.ctypes.data, T, wanted, produced, stop.size, stop.ctypes.data if stop.size else None, out.ctypes.data)
        a = SM.accept(c.tolist(), g.tolist())
        m, fired = SSM.stop_cut(g.tolist(), max(0, min(a + 1, wanted - produced)), set(stop.tolist()))
        assert out.tolist() == [a, m, int(fired)]


def test_the_probes_sample_is_the_sample_probes():
    rng, lib = np.random.default_rng(33), probe()
    for n in (1, 7, 300, 1000):
        v = (np.round(rng.standard_normal(n) * 4) / 4).astype(np.float32)
        for pos in range(16):
            sp = S(0.8, 40, 0.95, seed=77 + (pos << 33), stream=2)
            assert int(lib.ssp_sample(v.ctypes.data, n, sp.top_k, sp.temperature, sp.top_p, sp.seed, sp.stream, pos)) == c_sample(v, sp, pos)


# ── 2. the algorithm on the oracle ─────────────────────────────────────────────────────────────────────────────────────

N, START_TOKEN = 24, 3
FORMS = ["perfect", "wrong_everywhere", "wrong_at_two", "ngram"]
PARAMS = {"k40_p95": dict(temperature=0.8, top_k=40, top_p=0.95), "k256_p1": dict(temperature=1.5, top_k=256, top_p=1.0)}


def tiny():
    return llama.preset("tiny", 64)


def oracle_rows(oracle, T, sp, seen=None):
    """rows_fn of the model's loop: one execution of the token_len = T plan on the oracle, every logits row sampled by the header's
    rule at its own position. `seen` (a dict) receives position -> the row of every position whose candidates it was asked with."""
    cfg = tiny()
    m = llama.Model(cfg, llama.Q4_0, token_len=T)
    s = llama.Session(m, oracle.backend_fns())
    ob = oracle.OracleBackend()

    def rows(c, pos):
        s.prefill(c, pos, want_logits=False)
        logits = ob.buffer(s.handle, m.buf("logits"))[:T * cfg.vocab_size].reshape(T, cfg.vocab_size)
        if seen is not None:
            seen[pos] = (list(c), logits.copy())
        return [c_sample(logits[j], sp, pos + j) for j in range(T)]
    return rows, (s, m)


def drafts_of(form, stream, vocab):
    """drafts[i] = the guess for the token at position 1 + i (= stream[i]); None: n-gram lookup"""
    d = [int(t) for t in stream]
    wrong = {"perfect": (), "wrong_everywhere": range(len(d)), "wrong_at_two": (5, 14)}
    if form == "ngram":
        return None
    for i in wrong[form]:
        d[i] = (d[i] + 1) % vocab
    return d


def sequential(oracle, sp, n, greedy=False):
    """the oracle's sequential decode of the token_len = 1 plan from START_TOKEN at position 0: greedy, or every token sampled by
    the header's rule -> (tokens, the logits row of every position)"""
    m = llama.Model(tiny(), llama.Q4_0)
    s = llama.Session(m, oracle.backend_fns())
    tok, out, rows = START_TOKEN, [], []
    for pos in range(n):
        nxt, logits = s.step(tok, pos)
        tok = nxt if greedy else c_sample(logits, sp, pos)
        out.append(tok)
        rows.append(logits)
    s.close(), m.close()
    return out, rows


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("T", [2, 4])
def test_model_loop_on_the_oracle_gives_one_stream_whatever_the_drafts(oracle, T, name):
    sp = S(seed=1234, stream=1, **PARAMS[name])
    vocab = tiny().vocab_size
    rows, keep = oracle_rows(oracle, T, sp)
    # the stream, from a run without any draft (every candidate a pad): N + T - 1 tokens of it, so that perfect drafts exist for
    # the last step
    ref, n_ref, _ = SSM.spec_loop(rows, START_TOKEN, 0, N + T - 1, T, drafts=[])
    assert n_ref == N + T - 1 and len(set(ref)) > 3  # (it does sample)
    for form in FORMS:
        drafts = drafts_of(form, ref, vocab)
        toks, produced, stats = SSM.spec_loop(rows, START_TOKEN, 0, N, T, drafts=drafts)
        assert toks == ref[:N] and produced == N, form
        assert stats == SM.predict(ref, START_TOKEN, 0, N, T, drafts=drafts), form  # the acceptance bookkeeping is the greedy form's
        if form == "perfect":
            assert stats == {"steps": -(-N // T), "drafted": (T - 1) * -(-N // T), "accepted": (T - 1) * -(-N // T)}
        if form == "wrong_everywhere":
            assert stats == {"steps": N, "drafted": (T - 1) * N, "accepted": 0}
        if form == "wrong_at_two":
            assert -(-N // T) < stats["steps"] < N
    # a stop token in the middle of a step of the perfect run: the stream's prefix, and the same under useless drafts
    at = next(i for i in range(T, N) if ref[i] not in ref[:i] and i % T == (1 if T > 2 else 0))  # (the cut drops a token the step accepted)
    for form in ("perfect", "wrong_everywhere"):
        toks, produced, stats = SSM.spec_loop(rows, START_TOKEN, 0, N, T, drafts=drafts_of(form, ref, vocab), stop=[ref[at]])
        assert produced == at + 1 and toks == ref[:at + 1] + [-1] * (N - at - 1), form
        if form == "perfect":
            assert stats["steps"] == at // T + 1
    keep[0].close(), keep[1].close()


@pytest.mark.parametrize("T", [2, 4])
def test_top_k_1_is_the_sequential_greedy_stream(oracle, T):
    sp = S(temperature=0.7, top_k=1, seed=9)
    greedy, _ = sequential(oracle, sp, N + T - 1, greedy=True)
    rows, keep = oracle_rows(oracle, T, sp)
    for form in FORMS:
        drafts = drafts_of(form, greedy, tiny().vocab_size)
        toks, produced, stats = SSM.spec_loop(rows, START_TOKEN, 0, N, T, drafts=drafts)
        assert toks == greedy[:N] and produced == N, form
        assert stats == SM.predict(greedy, START_TOKEN, 0, N, T, drafts=drafts), form
    keep[0].close(), keep[1].close()


@pytest.mark.parametrize("T", [2, 4])
def test_equals_the_sequential_sampled_decode_where_the_rows_are_bit_equal(oracle, T):
    """The relation to zgml_hip_resident_decode_sampled on a token_len = 1 plan, on the oracle. THE CONDITION, asserted first and
    not a tolerance: at every compared position the T-plan's logits row and the decode plan's are bit-equal. Then the picks are
    the same function of the same bits at the same position, and the streams must be equal."""
    sp = S(seed=1234, stream=1, **PARAMS["k40_p95"])
    want, want_rows = sequential(oracle, sp, N + T - 1)
    seen = {}
    rows, keep = oracle_rows(oracle, T, sp, seen)
    toks, produced, _ = SSM.spec_loop(rows, START_TOKEN, 0, N, T, drafts=want)  # (perfect drafts if the streams are equal)
    at = [START_TOKEN] + want
    compared = 0
    for pos, (c, logits) in sorted(seen.items()):
        for j in range(T):
            if pos + j < N and c[:j + 1] == at[pos:pos + j + 1]:  # row j saw the sequential run's own context
                assert np.array_equal(logits[j], want_rows[pos + j]), f"condition: the T-plan's row of position {pos + j} is not the decode plan's"
                compared += 1
    assert compared >= N
    assert toks == want[:N] and produced == N
    keep[0].close(), keep[1].close()


# ── 3. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "spec_sampled_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DSPEC_SAMPLED_PROBE_MAIN", "-o", str(exe), str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "spec_sampled_probe ok" in r.stdout, r.stdout + r.stderr


# ── 4. the ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_speculative_sampled"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == 10  # ctx, program, first, start, n, opt, sampling, tokens_out, n_produced, stats
    assert name in (ROOT / "include" / "zgml_hip.h").read_text()
    assert hasattr(llama.Session, "resident_decode_speculative_sampled")
