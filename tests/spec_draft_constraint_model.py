"""A small Python model of speculative decode with a draft model under a constraint (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_speculative_model_constrained; the rule in zgml_amd/csrc/spec.h, DRAFTS FROM A MODEL UNDER A CONSTRAINT):
the draft's first maximum is taken over the tokens the walk's state allows, and the walk gives every verify row its state.
Everything behind the drafts — the acceptance rule, the dead-end cut, the stop cut, the state's advance — is imported from
tests/spec_model.py, tests/spec_sampled_model.py and tests/spec_constraint_model.py, not repeated.
tests/test_spec_draft_constraint_host.py holds spec.h to this file and runs the loop on the oracle;
tests/test_hip_spec_draft_constraint.py takes its references from it. Written from the contract, the slow and obvious way."""
import numpy as np

from tests import spec_model as SM
from tests import spec_sampled_model as SSM
from tests.spec_constraint_model import DEAD, NO_PICK, allowed_tokens, step_state


def masked_first_max(row, class_of, nxt, state):
    """the first maximum of `row` over the tokens `state` allows: the larger value wins, the lower index among equals, and the
    first allowed token when nothing beats it (a row of -inf); -1 when the state allows no token"""
    toks = allowed_tokens(class_of, nxt, state)  # ascending
    if toks.size == 0:
        return -1
    return int(toks[np.argmax(np.asarray(row)[toks])])  # (numpy's argmax is the first maximum; of a row of -inf, its first entry)


def draft_candidates(tok, T, state, class_of, nxt, draft_row, mask=True):
    """One step's candidates. draft_row(j, c) -> the logits row of the draft's execution j on c[j] (it stores the draft's KV column);
    all T executions run, the T-th for its column alone. mask=False is the rule WITHOUT the mask, for comparison: the draft's
    plain first maximum, which the state may forbid — the row behind it is then dead.
    -> (c, row_state, what `drafted` grows by, the executions' rows)"""
    c, row_state, rows = [int(tok)], [int(state)], []
    for j in range(T):
        row = draft_row(j, c)
        rows.append(row)
        if j == T - 1:
            break
        s = row_state[j]
        d = -1 if s == DEAD else masked_first_max(row, class_of, nxt, s) if mask else int(np.argmax(row))
        if d < 0:  # no draft: the token repeats, the row is dead
            c.append(c[j])
            row_state.append(DEAD)
        else:
            c.append(d)
            row_state.append(step_state(class_of, nxt, s, d))
    return c, row_state, sum(s != DEAD for s in row_state[1:]), rows


def spec_loop(rows_fn, draft_fn, first_token, start_pos, n_tokens, T, class_of, nxt, state, history=None, stop=(), mask=True, on_step=None):
    """The loop of the contract -> (tokens, n_produced, {"steps", "drafted", "accepted"}, the state afterwards); tokens has n_tokens
    entries, -1 behind a stop token or a dead end. rows_fn(c, pos, row_state, known) -> g[0..T-1] as in
    tests/spec_constraint_model.py: the target's constrained pick of every row under its state, NO_PICK without candidates.
    draft_fn(token, pos) -> the draft's logits row after one execution on `token` at `pos`.
    on_step(pos, c, row_state, g, a, m, draft_rows): once per step, for the conditions a test asserts on its reference."""
    known = [int(t) for t in history] if history is not None else []
    hist = known + [int(first_token)]
    stop = set(int(t) for t in stop)
    pos, out, stats, done = start_pos, [], {"steps": 0, "drafted": 0, "accepted": 0}, False
    while len(out) < n_tokens and not done:
        c, row_state, drafted, draft_rows = draft_candidates(hist[-1], T, state, class_of, nxt, lambda j, c: draft_fn(c[j], pos + j), mask)
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
        stats["steps"] += 1
        stats["drafted"] += drafted
        stats["accepted"] += a  # (before any cut)
        if on_step:
            on_step(pos, c, row_state, g, a, m, draft_rows)
        pos += m
    return out + [-1] * (n_tokens - len(out)), len(out), stats, state
