"""A float64 numpy model of constrained sampling (include/zgml_hip.h: zgml_token_dfa; the rule's text is THE CONSTRAINT of
zgml_amd/csrc/sample.h), written from the contract's text and sharing no code with the header. tests/test_constraint_host.py runs
the header (through tests/cpp/constraint_probe.cpp) against it.

The contract: a token that is not allowed in the current state is no candidate at all; the candidates are the
min(top_k, number of allowed tokens) largest logits among the allowed ones — value descending, the lower index first among equals,
-0 == +0, a NaN counts as -inf —; the pick is tests/sample_model.py's, whose MARGIN rule alone may set a case aside; the state
behind a token is next[state][class_of[token]]."""
import numpy as np

from tests import sample_model as M

FORBIDDEN = 0xFFFF


def allowed(class_of, next_table, state):
    """bool[vocab]: which tokens the state allows"""
    return np.asarray(next_table)[state][np.asarray(class_of)] != FORBIDDEN


def candidates(v, top_k, class_of, next_table, state):
    """indices of the candidates in order (an empty array: the state allows no token)"""
    idx = np.flatnonzero(allowed(class_of, next_table, state))
    if idx.size == 0:
        return idx
    return idx[M.candidates(np.asarray(v, np.float32)[idx], top_k)]


def pick(v, top_k, temperature, top_p, u, class_of, next_table, state):
    """-> (token or -1, rank, ambiguous, the state afterwards)"""
    cand = candidates(v, top_k, class_of, next_table, state)
    if cand.size == 0:
        return -1, -1, False, state
    rank, ambiguous = M.pick(np.asarray(v, np.float32)[cand], temperature, top_p, u)
    tok = int(cand[rank])
    return tok, rank, ambiguous, advance(class_of, next_table, state, tok)


def advance(class_of, next_table, state, token):
    return int(np.asarray(next_table)[state][np.asarray(class_of)[token]])


def penalized(v, recent, window, repeat, presence, frequency):
    """the logits the selection sees: float32, one rounded operation per line, over the last `window` of `recent` (which end with
    the token whose logits these are); a token >= n touches nothing"""
    f32 = np.float32
    out = np.array(v, f32)
    win = [t for t in list(recent)[-window:]] if window else []
    repeat = f32(1.0) if repeat == 0 else f32(repeat)
    inv = f32(1.0) / repeat
    with np.errstate(all="ignore"):
        for t in set(win):
            if t >= out.size:
                continue
            x = out[t]
            x = x * inv if x > 0 else x * repeat
            x = f32(x - f32(win.count(t)) * f32(frequency))
            out[t] = f32(x - f32(presence))
    return out
