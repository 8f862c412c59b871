"""CPU tests of constrained speculative decode under batching (include/zgml_hip.h:
zgml_hip_resident_decode_batch_speculative_constrained).

The lock-step model tests/batch_spec_constraint_model.py runs over the synthetic rows of tests/spec_constraint_model.py
(hashed_row: the logits row behind a token at a position, exact in float32): row b * Ts + j of a step is the row behind candidate
j of sequence b at its position + j, whatever the other sequences do. So every sequence of the batched model must equal the
single-sequence model run for that sequence ALONE — tests/spec_constraint_model.py's spec_loop for a sequence with an automaton,
tests/batch_spec_sampled_model.py's lockstep for one without —: tokens, count, statistics, final state. Every comparison is exact
equality of integers; the pick of a row is tests/cpp/constraint_probe.cpp's, which tests/test_constraint_host.py pins.

1. B = 3 at Ts = 2 / 4 / 5: a template automaton, a random automaton behind a history, an unattached sequence; perfect, n-gram,
   wrong-everywhere and no drafts rotate; with and without penalties.
2. Dead ends at the first pick and after k > 0 tokens; a stop token that advances the state; two ragged calls give the stream and
   the state of one.
3. What zgml_amd/csrc/spec.h states for the unattached sequence (kSpecRowFree, spec_free_rows, spec_row_selects), through
   tests/cpp/batch_spec_constraint_probe.cpp, against the model; the probe's stand-alone program under AddressSanitizer + UBSan.
4. The entry point is exported and declared in the ctypes mirror."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import batch_spec_constraint_model as BCM
from tests import batch_spec_sampled_model as BM
from tests import spec_constraint_model as SCM
from tests.test_constraint_host import random_dfa
from tests.test_spec_constraint_host import chain_dfa, model_rows, template_dfa
from tests.test_spec_sampled_host import drafts_of

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libbatch_spec_constraint_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "batch_spec_constraint_probe.cpp", ROOT / "zgml_amd" / "csrc" / "spec.h", ROOT / "zgml_amd" / "csrc" / "sample.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
u32 = np.uint32
S = capi.SamplingC.of
V, N = 200, 24
PARAMS = [dict(temperature=0.8, top_k=40, top_p=0.95, seed=1234, stream=0), dict(temperature=1.5, top_k=256, top_p=1.0, seed=77, stream=1),
          dict(temperature=1.1, top_k=64, top_p=0.9, seed=5 << 32, stream=2)]
PEN = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, penalty_window=16)
HISTORY = [(7 * i + 3) % V for i in range(4)]
FIRSTS, STARTS, COUNTS = [3, 90, 17], [0, len(HISTORY), 0], [N, 17, N]
TEMPLATE, _, TEMPLATE_LITS = template_dfa(V, [1, 3, 6], seed=9)
RANDOM = random_dfa(np.random.default_rng(5), V, n_states=6, n_classes=9, forbid=0.3)
ZERO = {"steps": 0, "drafted": 0, "accepted": 0}
_lib = None


def step_fn(Ts):
    """one execution of the synthetic batched plan: row b * Ts + j is the row behind token b * Ts + j at its sequence's position + j"""
    def step(tokens, positions):
        return np.stack([SCM.hashed_row(positions[r // Ts] + r % Ts, tokens[r], V) for r in range(len(tokens))])
    return step


def alone(rq, Ts):
    """the sequence by itself -> (tokens[rq.n], produced, statistics, state afterwards)"""
    if not rq.n:
        return [], 0, ZERO, rq.state if rq.dfa is not None else -1
    if rq.dfa is None:  # the sampled model, a batch of one
        toks, produced, stats, _ = BM.lockstep(step_fn(Ts), Ts, [BM.Request(rq.first, rq.start, rq.n, rq.sampling, history=rq.history, drafts=rq.drafts)])
        return toks[0].tolist(), produced[0], stats[0], -1
    return SCM.spec_loop(model_rows(V, rq.sampling, rq.dfa), rq.first, rq.start, rq.n, Ts, rq.dfa.class_of, rq.dfa.next, rq.state, history=rq.history,
                         drafts=rq.drafts, stop=rq.stop)


def check_against_alone(rqs, Ts, seqs_out=None):
    toks, produced, stats, _, states = BCM.lockstep(step_fn(Ts), Ts, rqs, seqs_out=seqs_out)
    for b, rq in enumerate(rqs):
        want = alone(rq, Ts)
        assert toks[b, :rq.n].tolist() == want[0] and np.all(toks[b, rq.n:] == -1), b
        assert (produced[b], stats[b], states[b]) == want[1:], (b, produced[b], stats[b], states[b], want[1:])
    return toks, produced, stats, states


def three(extra=({}, {}, {}), counts=COUNTS, drafts=(None, None, None), states=(0, 2, 0), dfas=(TEMPLATE, RANDOM, None)):
    hists = [None, HISTORY, None]
    return [BCM.Request(FIRSTS[b], STARTS[b], counts[b], S(**PARAMS[b], **extra[b]), history=hists[b], drafts=drafts[b], dfa=dfas[b], state=states[b])
            for b in range(3)]


# ── 1. every sequence equals its own loop ──────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("pen", [({}, {}, {}), (PEN, {}, PEN)], ids=["plain", "penalties"])
@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_every_sequence_equals_its_single_sequence_loop(Ts, pen):
    long = [n + Ts - 1 for n in COUNTS]
    seqs = []
    ref, n_ref, _, _ = check_against_alone(three(pen, counts=long, drafts=([], [], [])), Ts, seqs_out=seqs)
    assert n_ref == long  # precondition: no dead end on the way, perfect drafts exist for the last step
    streams = [ref[b, :long[b]].tolist() for b in range(3)]
    lits = set(sum(TEMPLATE_LITS, []))
    assert sum(t in lits for t in streams[0]) >= 8  # forced runs in sequence 0's stream
    assert all(f == SCM.NO_FORCED for f in seqs[1].frc) and len(set(streams[1])) > 3 and len(set(streams[2])) > 3  # the others sample
    assert seqs[0].stats["steps"] < long[0] and seqs[0].stats["drafted"] > 0  # without any draft the forced tokens still jump, and count as drafted
    assert seqs[2].stats["drafted"] == 0  # ... and nothing is ever placed for the unattached sequence
    forms = ["perfect", "ngram", "wrong_everywhere", "none"]
    for rot in range(4):
        fb = [forms[(b + rot) % 4] for b in range(3)]
        drafts = [[] if f == "none" else drafts_of(f, streams[b], V) for b, f in enumerate(fb)]
        for b in range(3):
            if fb[b] == "wrong_everywhere":
                assert all(d != t for d, t in zip(drafts[b], streams[b]))
        toks, produced, stats, states = check_against_alone(three(pen, drafts=drafts), Ts)
        for b in range(3):  # drafts, forced tokens and the batch decide the steps, never the tokens
            assert toks[b, :COUNTS[b]].tolist() == streams[b][:COUNTS[b]] and produced[b] == COUNTS[b], (fb, b)
            if fb[b] == "perfect":
                assert stats[b]["steps"] == -(-COUNTS[b] // Ts)
        # the unattached sequence: `drafted` is its mode's real drafts alone
        if fb[2] in ("perfect", "wrong_everywhere"):
            assert stats[2]["drafted"] == stats[2]["steps"] * (Ts - 1)
        if fb[2] == "none":
            assert stats[2]["drafted"] == 0
        assert states[2] == -1


# ── 2. dead ends, a stop token, two calls ──────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_dead_ends_at_the_first_pick_and_after_k_tokens(Ts):
    chain = chain_dfa(V, 7)  # every token is allowed, six times; state 6 allows none
    for state1, k in ((0, 6), (3, 3), (6, 0)):
        seqs = []
        toks, produced, stats, states = check_against_alone(three(dfas=(TEMPLATE, chain, None), states=(0, state1, 0)), Ts, seqs_out=seqs)
        assert produced == [N, k, N] and states[1] == 6 and seqs[1].dead_end and not seqs[0].dead_end and not seqs[2].dead_end
        assert np.all(toks[1, k:] == -1) and np.all(toks[1, :k] >= 0)
        if k == 0:
            assert stats[1]["steps"] == 1 and stats[1]["accepted"] == 0  # one step found it, then the sequence idled


def test_a_stop_token_cuts_its_sequence_and_advances_its_state():
    Ts = 4
    ref = check_against_alone(three(drafts=([], [], [])), Ts)[0]
    stream = ref[0].tolist()
    at = next(i for i in range(2, N) if stream[i] not in stream[:i] and i % Ts != Ts - 1)
    for drafts in (stream, [], None):
        toks, produced, stats, states = check_against_alone(three(extra=(dict(stop=[stream[at]]), {}, {}), drafts=(drafts, None, None)), Ts)
        assert produced == [at + 1, 17, N] and toks[0, :at + 1].tolist() == stream[:at + 1] and np.all(toks[0, at + 1:] == -1)
        state = 0
        for t in stream[:at + 1]:
            state = TEMPLATE.advance(state, t)
        assert states[0] == state  # over the stop token too
        assert toks[1].tolist() == ref[1].tolist() and toks[2].tolist() == ref[2].tolist()  # the others go on


@pytest.mark.parametrize("Ts", [2, 4, 5])
def test_two_ragged_calls_give_the_stream_and_the_state_of_one(Ts):
    one = check_against_alone(three(), Ts)
    cut = [10, 17, 3]  # sequence 1 has everything after the first call and idles through the second
    a = check_against_alone(three(counts=cut), Ts)
    rest = [COUNTS[b] - cut[b] for b in range(3)]
    rq2 = []
    for b in range(3):
        got = a[0][b, :cut[b]].tolist()
        hist = ([None, HISTORY, None][b] or []) + [FIRSTS[b]] + got[:-1]
        rq2.append(BCM.Request(got[-1], STARTS[b] + cut[b], rest[b], S(**PARAMS[b]), history=hist, dfa=(TEMPLATE, RANDOM, None)[b],
                               state=a[3][b] if a[3][b] >= 0 else 0))
    b2 = check_against_alone(rq2, Ts)
    for b in range(3):
        assert a[0][b, :cut[b]].tolist() + b2[0][b, :rest[b]].tolist() == one[0][b, :COUNTS[b]].tolist(), b
        assert b2[3][b] == one[3][b], b
    assert b2[2][1] == ZERO


# ── 3. the unattached sequence as spec.h states it ─────────────────────────────────────────────────────────────────────

def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", *FLAGS, "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, w = C.c_void_p, C.c_uint32
    lib.bscp_row_free.argtypes, lib.bscp_row_free.restype = [], w
    lib.bscp_free_rows.argtypes, lib.bscp_free_rows.restype = [vp, w], w
    lib.bscp_row_selects.argtypes, lib.bscp_row_selects.restype = [w], C.c_int
    lib.bscp_pass.argtypes, lib.bscp_pass.restype = [vp, w, w, w, w, vp, vp, w, vp, vp], w
    _lib = lib
    return lib


def c_pass(c, real, dfa, state, frc):
    c, row_state = np.ascontiguousarray(c, u32).copy(), np.zeros(len(c), u32)
    if dfa is None:
        placed = probe().bscp_pass(c.ctypes.data, c.size, real, 0, 0, None, None, 0, None, row_state.ctypes.data)
    else:
        frc = np.ascontiguousarray(frc, u32)
        placed = probe().bscp_pass(c.ctypes.data, c.size, real, 1, state, dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes, frc.ctypes.data,
                                   row_state.ctypes.data)
    return c.tolist(), row_state.tolist(), int(placed)


def test_the_free_row_is_the_models():
    lib = probe()
    assert lib.bscp_row_free() == BCM.FREE and BCM.FREE not in (SCM.DEAD, SCM.NO_PICK) and BCM.FREE > 0xFFFF  # no state of any automaton
    for s in (0, 1, 65534, BCM.FREE, SCM.DEAD):
        assert bool(lib.bscp_row_selects(s)) == BCM.row_selects(s)
    assert BCM.row_selects(BCM.FREE) and not BCM.row_selects(SCM.DEAD)
    rng = np.random.default_rng(81)
    for case in range(300):
        T = int(rng.integers(2, 9))
        real = int(rng.integers(0, T))
        c = rng.integers(0, V, T).tolist()
        assert c_pass(c, real, None, 0, None) == (c, *BCM.free_rows(T)), case  # candidates untouched, every row free, nothing placed
        dfa = random_dfa(rng, V, n_states=int(rng.integers(1, 7)), n_classes=int(rng.integers(1, 50)), forbid=float(rng.choice([0.3, 0.8, 0.95])))
        frc, state = SCM.forced(dfa.class_of, dfa.next), int(rng.integers(0, dfa.n_states))
        assert c_pass(c, real, dfa, state, frc) == SCM.constrain(c, real, state, dfa.class_of, dfa.next, frc), case  # ... beside an attached one


def test_probe_program_under_asan_ubsan():
    exe = BUILD / "batch_spec_constraint_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DBATCH_SPEC_CONSTRAINT_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "batch_spec_constraint_probe ok" in r.stdout, r.stdout + r.stderr


# ── 4. the ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_batch_speculative_constrained"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    assert getattr(lib, name).argtypes == lib.zgml_hip_resident_decode_batch_speculative_sampled.argtypes  # the signature of the sampled form
    assert name in (ROOT / "include" / "zgml_hip.h").read_text()
    assert hasattr(llama.BatchSession, "resident_decode_batch_speculative_constrained")
