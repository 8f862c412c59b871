"""A small Python model of speculative decode with a draft model (the contract in include/zgml_hip.h,
zgml_hip_resident_decode_speculative_model; the rule in zgml_amd/csrc/spec.h, DRAFTS FROM A MODEL): the loop that joins a target's
verify step with a draft's greedy steps. tests/test_spec_draft_model_host.py runs it on the oracle; tests/test_hip_spec_draft_model.py
predicts the device loop's tokens and statistics with it, and drives the host-side reference loops through it. Written from the
contract; the acceptance rule is tests/spec_model.py's."""
from tests import spec_model as SM


def spec_draft_loop(rows_fn, draft_fn, first_token, start_pos, n_tokens, T, stop=(), on_step=None):
    """rows_fn(candidates, pos) -> g[0..T-1], the token of every logits row of the target's verify step at `pos` (greedy or
    sampled: the caller's business). draft_fn(token, pos) -> the draft's greedy token after one execution on `token` at `pos`,
    which stores the draft's KV column `pos`. `stop`: tokens that end the call behind themselves (the sampled form).
    on_step(pos, c, g, a, m): called once per step, for the conditions a test asserts on its reference.
    -> (tokens, produced, {"steps", "drafted", "accepted"})"""
    tok, pos, out = int(first_token), start_pos, []
    stats = {"steps": 0, "drafted": 0, "accepted": 0}
    stopped = False
    while len(out) < n_tokens and not stopped:
        c = [tok]
        for j in range(T):  # the T-th execution is there for its KV column alone: its token is dropped
            d = int(draft_fn(c[j], pos + j))
            if j < T - 1:
                c.append(d)
        g = [int(t) for t in rows_fn(c, pos)]
        a = SM.accept(c, g)
        m = min(a + 1, n_tokens - len(out))
        for k in range(m):
            if g[k] in stop:
                m, stopped = k + 1, True
                break
        out += g[:m]
        tok, pos = g[m - 1], pos + m
        stats["steps"] += 1
        stats["drafted"] += T - 1
        stats["accepted"] += a
        if on_step:
            on_step(pos - m, c, g, a, m)
    return out, len(out), stats
