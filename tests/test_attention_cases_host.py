"""The expected side of tests/attention_cases.py, pinned on the CPU before any device runs: the oracle's attention against a
float64 softmax(Q K^T scale + mask) V for every case, and the skip rule on the oracle itself: non-finite K / V / scale values at
keys the reference skips leave its output bit-identical."""
import numpy as np
import pytest

from tests import attention_cases as AC

f32 = np.float32


def _buffers(be, h, prog):
    return {b: be.buffer(h, b).copy() for b in range(len(prog.buffer_sizes))}


@pytest.fixture(scope="module")
def clean_runs(oracle):
    """name -> outputs of the clean case on the oracle (computed once, never modified)"""
    cache = {}

    def get(name):
        if name not in cache:
            c = AC.build_case(name)
            cache[name] = AC.run_case(oracle.OracleBackend(), c)[0][0]
        return cache[name]
    return get


@pytest.mark.parametrize("name", AC.CASE_NAMES)
def test_oracle_matches_float64_softmax(oracle, name):
    """Bar 2e-6 (about five times the 3.6e-7 first measured over six shapes, d_head 4..320, seq_kv 90..5000). Measured over this
    table, every seq_kv of every case: max |oracle - float64| = 4.1e-7 (dense_dh64_dh128_first_tile_shut; the quantised-KV case 9.1e-8)."""
    c = AC.build_case(name)
    be = oracle.OracleBackend()
    h = be.compileProgram(c.prog)
    worst = 0.0
    try:
        for n in (None,) + tuple(c.refresh):
            if n is not None:
                be.refreshProgram(h, [o.with_(seq_kv=n) if o.kind in ("attention", "attention_kvq") else o for o in c.prog.ops])
            be.executeProgram(h, [], [])
            bufs = _buffers(be, h, c.prog)
            for op in c.attention_ops():
                want = AC.float64_attention(op, bufs, n)
                got = AC.gather_out(op, bufs[op.f["dst"]])
                assert np.isfinite(got).all()
                worst = max(worst, float(np.abs(got - want).max()))
    finally:
        be.freeProgram(h)
    print(f"{name}: max |oracle - float64| = {worst:.3g}")
    assert worst <= 2e-6


@pytest.mark.parametrize("variant", AC.VARIANTS)
@pytest.mark.parametrize("name", AC.SKIP_CASES)
def test_oracle_skips_poisoned_keys_bit_exactly(oracle, clean_runs, name, variant):
    c = AC.build_case(name, variant)
    got = AC.run_case(oracle.OracleBackend(), c)[0][0]
    want = AC.expected_of_variant(c, variant, clean_runs(name))
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_variants_poison_something_and_only_skipped_keys():
    """the table's own contract: each variant differs from the clean uploads, and K / V / scale poison sits on dead columns only"""
    for name in AC.SKIP_CASES:
        clean = AC.build_case(name)
        for variant in AC.VARIANTS:
            c = AC.build_case(name, variant)
            changed = [u.buf_idx for u, v in zip(clean.prog.initial_uploads, c.prog.initial_uploads)
                       if not np.array_equal(u.host.view(np.uint32), v.host.view(np.uint32))]
            assert changed, (name, variant)
            for op, dead in zip(c.attention_ops(), c.dead):
                if op.kind != "attention":
                    continue
                o = op.f
                for which in ("k", "v"):
                    buf = next(u.host for u in c.prog.initial_uploads if u.buf_idx == o[which])
                    rows = buf[o[which + "_off"] + np.arange(o["seq_kv"])[:, None] * o[which + "_cs"] + np.arange(o["d_head"])[None, :] * o[which + "_rs"]]
                    bad = np.flatnonzero(~np.isfinite(rows).all(axis=1))
                    assert set(bad) <= set(dead), (name, variant, which)
