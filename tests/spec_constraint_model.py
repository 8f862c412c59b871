"""A small Python model of constrained speculative decode (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_speculative_constrained): tests/spec_sampled_model.py's loop — draft rules, acceptance rule and stop cut
imported, not repeated — extended by the NEW INTEGER LOGIC alone: the forced token of a state, the pass that walks the automaton
over a step's candidates, the dead-end cut and the state's advance. The floating-point pick is not restated: rows_fn gets every
row's state and answers with the constrained pick of tests/cpp/constraint_probe.cpp (tests/test_constraint_host.py pins that one to
a float64 model). tests/test_spec_constraint_host.py holds zgml_amd/csrc/spec.h and sample_params.h to this file;
tests/test_hip_spec_constraint.py takes its references from it. Written from the contract, with Python lists."""
import numpy as np

from tests import spec_model as SM
from tests import spec_sampled_model as SSM

FORBIDDEN = 0xFFFF  # next[s][c]: not allowed
DEAD = 0xFFFF       # the state of a row that cannot be reached
NO_FORCED = 0xFFFFFFFF
NO_PICK = 0xFFFFFFFF  # g[j] of a row without candidates


def allowed_tokens(class_of, nxt, state):
    return np.flatnonzero(np.asarray(nxt)[state][np.asarray(class_of)] != FORBIDDEN)


def forced(class_of, nxt):
    """forced[s]: the single token state s allows when it allows exactly one token of the vocabulary, else NO_FORCED. Written the
    slow, obvious way — every state looks at every token —, not from per-class counts."""
    out = []
    for s in range(np.asarray(nxt).shape[0]):
        toks = allowed_tokens(class_of, nxt, s)
        out.append(int(toks[0]) if toks.size == 1 else NO_FORCED)
    return out


def step_state(class_of, nxt, state, token):
    """the state behind `token`, DEAD when it is not allowed"""
    return int(np.asarray(nxt)[state][np.asarray(class_of)[token]])


def constrain(c, real, state, class_of, nxt, frc):
    """the pass over the mode's candidates c (c[1..real] real drafts, pads behind them) from the sequence's state
    -> (candidates, row_state, forced tokens placed at pad positions)"""
    c, s, row_state, placed = list(c), state, [state], 0
    for j in range(1, len(c)):
        if s != DEAD:
            pad = j > real
            if frc[s] != NO_FORCED:
                c[j] = frc[s]  # also over a real draft
                placed += pad
            elif pad:
                c[j] = c[j - 1]  # re-evaluated: it may now follow a forced token
            s = step_state(class_of, nxt, s, c[j])
        row_state.append(s)
    return c, row_state, placed


def spec_loop(rows_fn, first_token, start_pos, n_tokens, T, class_of, nxt, state, history=None, drafts=None, ngram=2, stop=(), frc=None):
    """The loop of the contract -> (tokens, n_produced, {"steps", "drafted", "accepted"}, the state afterwards); tokens has
    n_tokens entries, -1 behind a stop token or a dead end. rows_fn(c, pos, row_state, known) -> g[0..T-1]: the constrained pick of
    every logits row under its state (known: the tokens at positions lo..pos, for a penalty window), NO_PICK for a row without
    candidates."""
    frc = forced(class_of, nxt) if frc is None else frc
    known = [int(t) for t in history] if history is not None else []
    lo = 0 if known else start_pos
    hist = known + [int(first_token)]
    assert len(hist) == start_pos - lo + 1
    stop = set(int(t) for t in stop)
    pos, out, stats, done = start_pos, [], {"steps": 0, "drafted": 0, "accepted": 0}, False
    while len(out) < n_tokens and not done:
        if drafts is not None:
            c, real = SM.candidates_provided(hist[-1], pos, start_pos, drafts, T)
        else:
            c, real = SM.candidates_lookup(hist, pos - lo, T, ngram)
        c, row_state, placed = constrain(c, real, state, class_of, nxt, frc)
        g = [int(t) for t in rows_fn(c, pos, row_state, list(hist))]
        assert all(g[j] == NO_PICK for j in range(T) if row_state[j] == DEAD)
        a = SM.accept(c, g)
        m = min(a + 1, n_tokens - len(out))
        if g[a] == NO_PICK:  # the reached state allows no token: cut in front of it, the call is finished
            m, done = min(m, a), True
        m, stopped = SSM.stop_cut(g, m, stop)
        done = done or stopped
        for t in g[:m]:
            state = step_state(class_of, nxt, state, t)
            assert state != DEAD
        out += g[:m]
        hist += g[:m]
        pos += m
        stats["steps"] += 1
        stats["drafted"] += real + placed
        stats["accepted"] += a  # (before any cut)
    return out + [-1] * (n_tokens - len(out)), len(out), stats, state


def hashed_row(pos, token, n):
    """the synthetic model of the host tests: the logits row behind `token` at position `pos`, multiples of 1/256 in [0, 256) from
    a 64-bit mix of (pos, token, index) — exact in float32, the same bits in tests/cpp/spec_constraint_probe.cpp"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((pos * 0x10001 + token * 0x3D + 7) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(20)) & np.uint64(0xFFFF)).astype(np.float32) / np.float32(256.0)
