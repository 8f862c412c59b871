"""CPU tests of constrained speculative decode (include/zgml_hip.h: zgml_hip_resident_decode_speculative_constrained). The rule is
zgml_amd/csrc/spec.h (UNDER A CONSTRAINT: spec_constrain_candidates, spec_dead_end_cut, spec_state_advance) and
zgml_amd/csrc/sample_params.h (constraint_forced) — the functions the kernels and the runtime call —, reached through
tests/cpp/spec_constraint_probe.cpp. Every comparison is exact equality of integers; the floating-point pick is
tests/cpp/constraint_probe.cpp's, which tests/test_constraint_host.py pins.

1. forced[] against the model tests/spec_constraint_model.py: random automata and the hand-made states with 0, 1 and 2 allowed
   tokens, an empty class, a singleton class beside an empty one.
2. The pass over a step's candidates against the model: c, row_state and the `drafted` increment, T in 2..8; forced over a real
   draft, pad re-propagation behind a forced token, a forbidden draft killing every later row.
3. The whole loop — the probe's, in the order the launches apply the rules — against the model's loop over the same synthetic
   rows: tokens, produced, statistics and final state; a dead end at row 0 and one in the middle of a step.
4. The probe's stand-alone program under AddressSanitizer + UBSan.
5. The entry point is exported and declared in the ctypes mirror."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_constraint_model as SCM
from tests.test_constraint_host import Dfa, FORBIDDEN, c_constraint_sample, random_dfa

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libspec_constraint_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "spec_constraint_probe.cpp", ROOT / "tests" / "cpp" / "constraint_probe.cpp", ROOT / "zgml_amd" / "csrc" / "spec.h",
        ROOT / "zgml_amd" / "csrc" / "sample.h", ROOT / "zgml_amd" / "csrc" / "sample_params.h", ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
u16, u32 = np.uint16, np.uint32
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
    vp, w, u64, fl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    for name in ("scp_no_pick", "scp_no_forced", "scp_dead"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [], w
    lib.scp_forced.argtypes, lib.scp_forced.restype = [C.POINTER(capi.TokenDfaC), vp], C.c_int
    lib.scp_constrain.argtypes, lib.scp_constrain.restype = [vp, w, w, w, vp, vp, w, vp, vp], w
    lib.scp_loop.argtypes = [w, w, w, w, w, vp, w, w, vp, w, w, vp, w, fl, w, fl, u64, w, fl, fl, fl, w, C.POINTER(capi.TokenDfaC), C.POINTER(w), vp, vp]
    lib.scp_loop.restype = w
    _lib = lib
    return lib


def dfa_c(dfa):
    d = capi.TokenDfaC()
    d.n_states, d.n_classes, d.vocab = dfa.n_states, dfa.n_classes, dfa.class_of.size
    d.class_of, d.next = dfa.class_of.ctypes.data_as(C.POINTER(C.c_uint16)), dfa.next.ctypes.data_as(C.POINTER(C.c_uint16))
    return d


def c_forced(dfa):
    out = np.zeros(dfa.n_states, u32)
    assert probe().scp_forced(C.byref(dfa_c(dfa)), out.ctypes.data) == 0
    return out.tolist()


def c_constrain(c, real, state, dfa, frc):
    c, frc, row_state = np.ascontiguousarray(c, u32).copy(), np.ascontiguousarray(frc, u32), np.zeros(len(c), u32)
    placed = probe().scp_constrain(c.ctypes.data, c.size, real, state, dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes, frc.ctypes.data,
                                   row_state.ctypes.data)
    return c.tolist(), row_state.tolist(), int(placed)


def test_the_sentinels_are_the_models():
    lib = probe()
    assert (lib.scp_no_pick(), lib.scp_no_forced(), lib.scp_dead()) == (SCM.NO_PICK, SCM.NO_FORCED, SCM.DEAD)
    assert SCM.NO_PICK >= 1 << 31 and SCM.DEAD == FORBIDDEN


# ── 1. forced[] ────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_forced_cases_by_hand():
    # tokens 0..5; classes: 0 = {0, 1}, 1 = {2}, 2 = {} (empty), 3 = {3}, 4 = {4, 5}
    class_of = [0, 0, 1, 3, 4, 4]
    F = FORBIDDEN
    nxt = [[F, F, F, F, F],   # no token
           [F, 0, F, F, F],   # one: the singleton class 1 -> token 2
           [F, 0, 0, F, F],   # the singleton beside the allowed EMPTY class 2: still forced
           [F, F, 0, F, F],   # the empty class alone: no token
           [F, 0, F, 0, F],   # two singleton classes: two tokens
           [0, F, F, F, F],   # one class of two tokens
           [F, F, 1, 2, F]]   # the empty class in front of a singleton: token 3
    dfa = Dfa(class_of, np.array(nxt, u16))
    want = [SCM.NO_FORCED, 2, 2, SCM.NO_FORCED, SCM.NO_FORCED, SCM.NO_FORCED, 3]
    assert SCM.forced(dfa.class_of, dfa.next) == want  # the model, by counting tokens
    assert c_forced(dfa) == want


def test_forced_matches_the_model_on_random_automata():
    rng = np.random.default_rng(71)
    seen = {"none": 0, "one": 0, "more": 0}
    for case in range(300):
        vocab, n_classes = int(rng.integers(1, 60)), int(rng.integers(1, 80))  # (more classes than tokens: empty and singleton classes)
        dfa = random_dfa(rng, vocab, n_states=int(rng.integers(1, 7)), n_classes=n_classes, forbid=float(rng.choice([0.3, 0.8, 0.97])))
        want = SCM.forced(dfa.class_of, dfa.next)
        assert c_forced(dfa) == want, case
        for s in range(dfa.n_states):
            k = int(dfa.allowed(s).sum())
            seen["none" if k == 0 else "one" if k == 1 else "more"] += 1
            assert (want[s] != SCM.NO_FORCED) == (k == 1)
    assert all(v >= 50 for v in seen.values()), seen


# ── 2. the pass ────────────────────────────────────────────────────────────────────────────────────────────────────────

def template_dfa(vocab, runs, free_classes=3, seed=0):
    """A template automaton: free states — every token of `free_classes` hashed classes is allowed — alternate with literal runs of
    runs[i] forced tokens (each a singleton class of its own); behind the last run the walk returns to the first free state.
    -> (Dfa, the free states, the literal tokens of every run)"""
    rng = np.random.default_rng(seed)
    n_lit = sum(runs)
    lits = rng.choice(vocab, n_lit, replace=False).tolist()
    class_of = (np.arange(vocab) % free_classes).astype(u16)
    for i, t in enumerate(lits):
        class_of[t] = free_classes + i
    n_states = len(runs) + n_lit
    nxt = np.full((n_states, free_classes + n_lit), FORBIDDEN, u16)
    state, free, lit_at, k = 0, [], [], 0
    for r in runs:
        free.append(state)
        nxt[state, :free_classes] = state + 1 if r else (state + 1) % n_states  # any free token starts the run
        run = []
        for _ in range(r):
            state += 1
            nxt[state, free_classes + k] = (state + 1) % n_states
            run.append(lits[k])
            k += 1
        lit_at.append(run)
        state += 1
    return Dfa(class_of, nxt), free, lit_at


def test_pass_cases_by_hand():
    dfa, free, lits = template_dfa(64, [3, 1], seed=5)
    frc = SCM.forced(dfa.class_of, dfa.next)
    a, b, c3 = lits[0]
    assert frc[:5] == [SCM.NO_FORCED, a, b, c3, SCM.NO_FORCED] and free == [0, 4]
    free_tok = next(t for t in range(64) if t not in sum(lits, []))
    other = next(t for t in range(64) if t not in sum(lits, []) and t != free_tok)
    # forced overrides a real draft: from state 1 the drafts 7, 7, 7 (T = 4, all real) become the run
    for fn in (lambda *x: SCM.constrain(*x[:3], dfa.class_of, dfa.next, frc), lambda *x: c_constrain(*x[:3], dfa, frc)):
        assert fn([free_tok, other, other, other], 3, 1) == ([free_tok, a, b, c3], [1, 2, 3, 4], 0)
        # pads behind a forced token: no real draft, the pads become the run and count as drafted; behind the run the state is free
        # again and the pad repeats the run's last token — re-propagated, not the mode's pad free_tok —, which that state forbids:
        # the last row is dead and its candidate stays the mode's
        assert fn([free_tok] * 6, 0, 1) == ([free_tok, a, b, c3, c3, free_tok], [1, 2, 3, 4, SCM.DEAD, SCM.DEAD], 3)
        # a forbidden draft kills every later row: in the free state 0 the literal `a` is not allowed
        assert fn([free_tok, a, free_tok, free_tok], 3, 0) == ([free_tok, a, free_tok, free_tok], [0, SCM.DEAD, SCM.DEAD, SCM.DEAD], 0)
        # an allowed draft in a free state stays, and the forced run behind it replaces the next drafts
        assert fn([free_tok, other, other, other, other], 4, 0) == ([free_tok, other, a, b, c3], [0, 1, 2, 3, 4], 0)
        # one real draft, then pads: the forced tokens at pad positions count
        assert fn([free_tok, other, other, other, other], 1, 0) == ([free_tok, other, a, b, c3], [0, 1, 2, 3, 4], 3)


def test_pass_matches_the_model_on_random_cases():
    rng = np.random.default_rng(72)
    seen = {"forced_over_draft": 0, "pad_behind_forced": 0, "killed": 0, "untouched": 0}
    for case in range(4000):
        vocab = int(rng.integers(2, 40))
        dfa = random_dfa(rng, vocab, n_states=int(rng.integers(1, 7)), n_classes=int(rng.integers(1, 50)), forbid=float(rng.choice([0.3, 0.8, 0.95])))
        frc = SCM.forced(dfa.class_of, dfa.next)
        T = int(rng.integers(2, 9))
        real = int(rng.integers(0, T))
        c = [int(rng.integers(0, vocab))]
        for j in range(1, T):
            c.append(int(rng.integers(0, vocab)) if j <= real else c[-1])
        state = int(rng.integers(0, dfa.n_states))
        want = SCM.constrain(c, real, state, dfa.class_of, dfa.next, frc)
        assert c_constrain(c, real, state, dfa, frc) == want, case
        wc, ws, placed = want
        seen["forced_over_draft"] += any(wc[j] != c[j] for j in range(1, real + 1))
        seen["pad_behind_forced"] += any(j > real and ws[j - 1] != SCM.DEAD and frc[ws[j - 1]] == SCM.NO_FORCED and wc[j - 1] != c[j - 1] and wc[j] == wc[j - 1]
                                         for j in range(2, T))
        seen["killed"] += SCM.DEAD in ws and ws[-1] == SCM.DEAD and ws.count(SCM.DEAD) >= 2
        seen["untouched"] += wc == c
        assert placed == sum(1 for j in range(real + 1, T) if ws[j - 1] != SCM.DEAD and frc[ws[j - 1]] != SCM.NO_FORCED)
    assert all(v >= 30 for v in seen.values()), seen


# ── 3. the whole loop ──────────────────────────────────────────────────────────────────────────────────────────────────

def model_rows(vocab, sp, dfa):
    """rows_fn of the model's loop over the synthetic model: row j is hashed_row(pos + j, c[j]), picked by the existing probe under
    the row's state with the verify step's window"""
    def rows(c, pos, row_state, known):
        g = []
        for j in range(len(c)):
            if row_state[j] == SCM.DEAD:
                g.append(SCM.NO_PICK)
                continue
            tok, _ = c_constraint_sample(SCM.hashed_row(pos + j, c[j], vocab), sp, pos + j, known + c[1:j + 1], dfa, row_state[j])
            g.append(tok if tok >= 0 else SCM.NO_PICK)
        return g
    return rows


def c_loop(vocab, first, start, n, T, sp, dfa, state, history=None, drafts=None, ngram=2, stop=()):
    hist = np.ascontiguousarray([] if history is None else history, u32)
    dr = np.ascontiguousarray([] if drafts is None else drafts, u32)
    st = np.ascontiguousarray(stop, u32)
    toks, stats, state_io = np.zeros(max(1, n), np.int64), np.zeros(3, u32), C.c_uint32(state)
    made = probe().scp_loop(vocab, first, start, n, T, hist.ctypes.data if hist.size else None, hist.size, 0 if drafts is None else 1,
                            dr.ctypes.data if dr.size else None, dr.size, ngram, st.ctypes.data if st.size else None, st.size, sp.temperature, sp.top_k, sp.top_p,
                            sp.seed, sp.stream, sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty, sp.penalty_window, C.byref(dfa_c(dfa)),
                            C.byref(state_io), toks.ctypes.data, stats.ctypes.data)
    return toks[:n].tolist(), int(made), dict(zip(("steps", "drafted", "accepted"), (int(x) for x in stats))), int(state_io.value)


def both_loops(vocab, first, start, n, T, sp, dfa, state, **kw):
    want = SCM.spec_loop(model_rows(vocab, sp, dfa), first, start, n, T, dfa.class_of, dfa.next, state, **kw)
    got = c_loop(vocab, first, start, n, T, sp, dfa, state, **kw)
    assert got == want, (got, want)
    return want


PEN = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, penalty_window=16)


def test_loop_matches_the_model_on_a_template_and_on_random_automata():
    vocab = 200
    dfa, free, lits = template_dfa(vocab, [1, 3, 6], seed=9)
    n_forced = 0
    for T in (2, 4, 5, 8):
        for pen in ({}, PEN):
            sp = S(0.8, 40, 0.95, seed=11 + T, stream=1, **pen)
            ref, produced, stats, state = both_loops(vocab, 3, 0, 24, T, sp, dfa, 0, drafts=[])
            assert produced == 24 and stats["steps"] < 24  # forced runs are jumped over without any draft
            flat = sum(lits, [])
            n_forced += sum(t in flat for t in ref)
            for drafts in (None, ref, [(t + 1) % vocab for t in ref], []):  # n-gram, perfect, wrong everywhere, none
                toks, p2, st2, state2 = both_loops(vocab, 3, 0, 24, T, sp, dfa, 0, drafts=drafts)
                assert (toks, p2, state2) == (ref, produced, state)  # drafts change the step count alone
            a = both_loops(vocab, 3, 0, 10, T, sp, dfa, 0)
            b = both_loops(vocab, a[0][9], 10, 14, T, sp, dfa, a[3], history=[3] + a[0][:9])
            assert a[0] + b[0] == ref and b[3] == state  # two calls equal one
            stop = ref[7]
            cut = both_loops(vocab, 3, 0, 24, T, sp, dfa, 0, drafts=ref, stop=[stop])
            assert cut[1] == ref.index(stop) + 1 and cut[0][:cut[1]] == ref[:cut[1]]
    assert n_forced > 100
    rng = np.random.default_rng(73)
    ended = {"dead_end": 0, "full": 0}
    for case in range(120):
        v = int(rng.integers(20, 120))
        d = random_dfa(rng, v, n_states=int(rng.integers(2, 7)), n_classes=int(rng.integers(2, 40)), forbid=float(rng.choice([0.5, 0.85])))
        T, n = int(rng.integers(2, 9)), int(rng.integers(1, 20))
        start = int(rng.integers(0, 4))
        hist = rng.integers(0, v, start).tolist() if rng.random() < 0.5 else None
        drafts = rng.integers(0, v, int(rng.integers(0, 25))).tolist() if rng.random() < 0.6 else None
        sp = S(1.2, int(rng.choice([1, 5, 40])), 0.9, seed=int(rng.integers(0, 1 << 40)), stream=case, **(PEN if case % 3 == 0 else {}))
        want = both_loops(v, int(rng.integers(0, v)), start, n, T, sp, d, int(rng.integers(0, d.n_states)), history=hist, drafts=drafts)
        ended["full" if want[1] == n else "dead_end"] += 1
    assert all(x >= 20 for x in ended.values()), ended


def chain_dfa(vocab, n_states, token_of=None):
    """state s leads to s + 1; the last state allows no token. token_of: state -> its only token (None: every token is allowed)"""
    nxt = np.full((n_states, 1 if token_of is None else vocab), FORBIDDEN, u16)
    for s in range(n_states - 1):
        nxt[s, 0 if token_of is None else token_of(s)] = s + 1
    return Dfa(np.zeros(vocab, u16) if token_of is None else np.arange(vocab, dtype=u16), nxt)


def test_dead_ends_at_row_0_and_in_the_middle_of_a_step():
    vocab, T, sp = 64, 4, S(0.8, 40, 0.95, seed=5)
    free = both_loops(vocab, 3, 0, 12, T, sp, chain_dfa(vocab, 40), 0, drafts=[])[0]
    dfa = chain_dfa(vocab, 7)  # six tokens are left from state 0
    # perfect drafts: step 1 emits 4, step 2 reaches the dead end at its row 2 and emits 2
    toks, produced, stats, state = both_loops(vocab, 3, 0, 12, T, sp, dfa, 0, drafts=free)
    assert (produced, state, stats["steps"]) == (6, 6, 2) and toks == free[:6] + [-1] * 6
    # at row 0 of the first step: nothing, one step, the state stays
    toks, produced, stats, state = both_loops(vocab, 3, 0, 12, T, sp, dfa, 6, drafts=free)
    assert (produced, state, stats) == (0, 6, {"steps": 1, "drafted": 3, "accepted": 0}) and toks == [-1] * 12
    # a fully forced chain: the tokens are the chain whatever the drafts say, T per step
    forced_chain = chain_dfa(vocab, 30, token_of=lambda s: (7 * s + 1) % vocab)
    toks, produced, stats, state = both_loops(vocab, 3, 0, 24, T, sp, forced_chain, 0, drafts=[63] * 40)
    assert toks == [(7 * s + 1) % vocab for s in range(24)] and (produced, state, stats["steps"]) == (24, 24, 6)


# ── 4. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "spec_constraint_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSPEC_CONSTRAINT_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "spec_constraint_probe ok" in r.stdout, r.stdout + r.stderr


# ── 5. the ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_speculative_constrained"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    assert getattr(lib, name).argtypes == lib.zgml_hip_resident_decode_speculative_sampled.argtypes  # the signature of the sampled form
    assert name in (ROOT / "include" / "zgml_hip.h").read_text()
    assert hasattr(llama.Session, "resident_decode_speculative_constrained")
