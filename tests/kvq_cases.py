"""Shared by the GPU tests of batched decode over int8 KV caches (tests/test_hip_batch_kvq.py, tests/test_hip_kv_move.py): the
models, the bound and the both-backends stepping loop.

The bound. An int8 cache column on the device may differ from the oracle's by whole quantisation units: storeColumn TRUNCATES
v * 127 / max, so a 1-ulp difference in a projected key / value (the mat-vec's summation order) that straddles an integer moves
the cached byte by one. Logits are therefore held to 1e-3 of the row's largest magnitude, the bound tests/test_hip_kvq.py and
tests/test_hip_l7dims.py use for int8 caches; greedy tokens must agree wherever the oracle's own top-two gap exceeds twice that
bound (a closer pair may legitimately swap), and at least 90 % of the (step, sequence) rows must be such rows — the seeds below
were chosen on the CPU so that the oracle alone meets that."""
import numpy as np

from zgml_amd import llama

KVQ_TOL = 1e-3


def tiny64():
    """the tiny preset with two heads of 64 dims over one kv head: two 32-blocks per cache column"""
    cfg = llama.preset("tiny")
    cfg.n_heads, cfg.n_kv_heads = 2, 1
    return cfg


def decisive(l_ref_row):
    """the oracle's top-two logit gap of this row exceeds twice the bound"""
    top = np.sort(l_ref_row)[-2:]
    return bool(top[1] - top[0] > 2 * KVQ_TOL * np.abs(l_ref_row).max())


def oracle_trace(s_ref, tokens, positions, n_steps):
    """the oracle's greedy run: [(tokens, positions, logits, next)] per step"""
    toks, pos, trace = np.array(tokens), np.array(positions), []
    for _ in range(n_steps):
        t_ref, l_ref = s_ref.step(toks, pos)
        trace.append((toks.copy(), pos.copy(), l_ref, t_ref))
        toks, pos = t_ref.copy(), pos + 1
    return trace


def check_against_trace(be, s_hip, trace):
    """Step the HIP session over the oracle's tokens: every logit within KVQ_TOL of the row's largest magnitude, equal greedy tokens
    on the decisive rows, and at least 90 % of the rows decisive. Every row is stepped and printed before anything is asserted.
    -> (worst relative difference, decisive rows, rows)"""
    worst, n_dec, n_rows, off, swapped = 0.0, 0, 0, [], []
    for step, (toks, pos, l_ref, t_ref) in enumerate(trace):
        t_hip, l_hip = s_hip.step(toks, pos)
        assert not be.last_error(), be.last_error()
        assert np.isfinite(l_hip).all()
        for b in range(len(toks)):
            rel = float(np.abs(l_hip[b] - l_ref[b]).max() / np.abs(l_ref[b]).max())
            worst = max(worst, rel)
            print(f"step {step} seq {b}: rel {rel:.3g} decisive {decisive(l_ref[b])} tokens {int(t_hip[b])} {int(t_ref[b])}")
            n_rows += 1
            if rel > KVQ_TOL:
                off.append((step, b, rel))
            if decisive(l_ref[b]):
                n_dec += 1
                if int(t_hip[b]) != int(t_ref[b]):
                    swapped.append((step, b))
    assert not off, off
    assert not swapped, swapped
    assert n_dec >= 0.9 * n_rows, (n_dec, n_rows)
    return worst, n_dec, n_rows
