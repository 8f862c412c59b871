"""A small Python model of greedy-exact speculative decode (the contract in include/zgml_hip.h, zgml_hip_resident_decode_speculative):
the draft rules, the acceptance rule and the loop. tests/test_spec_decode_host.py holds zgml_amd/csrc/spec.h to it and runs it
on the oracle; tests/test_hip_spec_decode.py predicts the device loop's statistics with it. Written from the contract, with
Python lists and slices — deliberately not in the shape of the C++."""
import numpy as np


def lookup(hist, pos, ngram):
    """The match position of an n-gram lookup over hist[0..pos], or None: n = ngram .. 1, the first n that has an earlier
    occurrence of the last n tokens wins, and among its occurrences the latest."""
    for n in range(ngram, 0, -1):
        if n > pos + 1:
            continue
        suffix = list(hist[pos - n + 1:pos + 1])
        for i in range(pos - 1, n - 2, -1):
            if list(hist[i - n + 1:i + 1]) == suffix:
                return i
    return None


def candidates_lookup(hist, pos, T, ngram):
    """-> (the T candidates, real drafts among them)"""
    i = lookup(hist, pos, ngram)
    if i is None:
        return [int(hist[pos])] * T, 0
    v = [int(t) for t in hist[:pos + 1]]
    for k in range(T - 1):
        v.append(v[i + 1 + k])  # the history followed by the drafts chosen so far
    return v[pos:pos + T], T - 1


def candidates_provided(tok, pos, start_pos, drafts, T):
    c, real = [int(tok)], 0
    for j in range(1, T):
        x = pos + j - start_pos - 1
        if 0 <= x < len(drafts):
            c.append(int(drafts[x]))
            real += 1
        else:
            c.append(c[-1])
    return c, real


def accept(c, g):
    a = 0
    while a + 1 < len(c) and c[a + 1] == g[a]:
        a += 1
    return a


def spec_loop(rows_fn, first_token, start_pos, n_tokens, T, history=None, drafts=None, ngram=2):
    """The loop of the contract. rows_fn(candidates, pos) -> g[0..T-1], the greedy token of every logits row of a verify step.
    -> (tokens, {"steps", "drafted", "accepted"})"""
    known = [int(t) for t in history] if history is not None else []
    lo = 0 if known else start_pos  # first position the history knows
    hist = known + [int(first_token)]
    assert len(hist) == start_pos - lo + 1
    pos, out, stats = start_pos, [], {"steps": 0, "drafted": 0, "accepted": 0}
    while len(out) < n_tokens:
        if drafts is not None:
            c, real = candidates_provided(hist[-1], pos, start_pos, drafts, T)
        else:
            c, real = candidates_lookup(hist, pos - lo, T, ngram)
        g = [int(t) for t in rows_fn(c, pos)]
        a = accept(c, g)
        m = min(a + 1, n_tokens - len(out))
        out += g[:m]
        hist += g[:m]
        pos += m
        stats["steps"] += 1
        stats["drafted"] += real
        stats["accepted"] += a
    return out, stats


def stream_rows(stream, first_token, start_pos):
    """rows_fn over a known greedy stream (stream[i] = the token at position start_pos + 1 + i given everything before it): row j is
    known as long as the candidates c[0..j] are the stream's own tokens — which is all the acceptance rule ever looks at."""
    at = [int(first_token)] + [int(t) for t in stream]  # at[p - start_pos] = the token at position p

    def rows(c, pos):
        g, on_stream = [], True
        for j in range(len(c)):
            on_stream = on_stream and c[j] == at[pos + j - start_pos]
            g.append(at[pos + j + 1 - start_pos] if on_stream else -1)  # (IndexError: the stream handed over is too short)
        return g
    return rows


def predict(stream, first_token, start_pos, n_tokens, T, history=None, drafts=None, ngram=2):
    """What the loop must produce and count when the model's greedy continuation is `stream` (n_tokens + T - 1 tokens of it)."""
    toks, stats = spec_loop(stream_rows(stream, first_token, start_pos), first_token, start_pos, n_tokens, T, history, drafts, ngram)
    assert toks == [int(t) for t in stream[:n_tokens]]
    return stats


def top2_gap(logits):
    """(top1 - top2) / max |logit| of one logits row"""
    l = np.asarray(logits, np.float64)
    top = np.partition(l, -2)[-2:]
    return float(top[1] - top[0]) / float(np.abs(l).max())
