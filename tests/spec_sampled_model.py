"""A small Python model of sampled speculative decode (the contract in include/zgml_hip.h, zgml_hip_resident_decode_speculative_sampled):
tests/spec_model.py's loop — its draft rules and its acceptance rule, imported, not repeated — plus the stop cut. rows_fn gives the
SAMPLED token of every logits row (row j at position pos + j). tests/test_spec_sampled_host.py holds zgml_amd/csrc/spec.h's cut to
stop_cut and runs the loop on the oracle; tests/test_hip_spec_sampled.py takes its reference and its statistics from it. Written
from the contract, with Python lists and slices."""
from tests import spec_model as SM


def stop_cut(g, m, stop):
    """Among the tokens a step would emit, g[:m], the first stop token ends the emission behind itself
    -> (tokens emitted, a stop fired)"""
    for k, t in enumerate(g[:m]):
        if t in stop:
            return k + 1, True
    return m, False


def spec_loop(rows_fn, first_token, start_pos, n_tokens, T, history=None, drafts=None, ngram=2, stop=()):
    """The loop of the contract -> (tokens, n_produced, {"steps", "drafted", "accepted"}); tokens has n_tokens entries, -1 behind
    a stop token."""
    known = [int(t) for t in history] if history is not None else []
    lo = 0 if known else start_pos  # first position the history knows
    hist = known + [int(first_token)]
    assert len(hist) == start_pos - lo + 1
    stop = set(int(t) for t in stop)
    pos, out, stats, stopped = start_pos, [], {"steps": 0, "drafted": 0, "accepted": 0}, False
    while len(out) < n_tokens and not stopped:
        if drafts is not None:
            c, real = SM.candidates_provided(hist[-1], pos, start_pos, drafts, T)
        else:
            c, real = SM.candidates_lookup(hist, pos - lo, T, ngram)
        g = [int(t) for t in rows_fn(c, pos)]
        a = SM.accept(c, g)
        m, stopped = stop_cut(g, min(a + 1, n_tokens - len(out)), stop)
        out += g[:m]
        hist += g[:m]
        pos += m
        stats["steps"] += 1
        stats["drafted"] += real
        stats["accepted"] += a  # (before any cut)
    return out + [-1] * (n_tokens - len(out)), len(out), stats
