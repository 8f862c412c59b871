"""tests/decode_attention_cases.py pinned on the CPU before any device runs: the restated rules give every instantiation the
launchers reach and every cut of each; each mask variant kills exactly the wave, slot, round or chunk it names; the float64
reference agrees with the oracle on every clean step; the oracle's own poisoned run is bit-equal to its clean run."""
import time

import numpy as np
import pytest

from tests import decode_attention_cases as DC

f32 = np.float32


def test_restated_forms():
    """the instantiations of kernels_generic.hip launch_attention_decode_batch and of the two fused launches (qmatvec.hip)"""
    F = DC.decode_form
    assert [(f.lpk, f.block, f.kpw, f.full) for f in map(lambda d: F(d, False), DC.F32_D_HEADS)] == \
        [(2, 1024, 32, 2048), (4, 1024, 16, 1024), (8, 1024, 8, 512), (16, 1024, 4, 256), (32, 256, 2, 32), (64, 1024, 1, 64)]
    assert (F(64, False, 256).block, F(64, False, 256).full) == (256, 64) and (F(128, False, 1024).block, F(128, False, 1024).full) == (1024, 128)
    assert F(8, False, 256).block == 1024 and F(256, False, 256).block == 1024  # a forced size moves d_head 64 and 128 only
    assert [(f.q16, f.lpkm, f.kpw, f.keys_per_wave, f.full) for f in map(lambda d: F(d, True), DC.KVQ_D_HEADS)] == \
        [(False, 8, 8, 32, 512), (False, 16, 4, 16, 256), (True, 8, 8, 8, 512), (True, 16, 4, 4, 256)]
    assert F(16, True) is None and F(4, False) is None and F(512, False) is None
    assert max(DC.cut_lengths(F(8, False)).values()) == 4097 and max(DC.cut_lengths(F(256, False)).values()) == 129
    b = DC.body_form(128, True, 256)  # <32, true, 256>: the K-on-lanes launch only
    assert (b.q16, b.max_waves, b.full) == (True, 4, 128)


def test_restated_rounds_and_split():
    f = DC.decode_form(64, False)  # KPW 4, U 4, 16 waves
    assert DC.rounds(1, f) == (1, 4, 16, 1, (0,)) and DC.rounds(16, f)[0] == 1 and DC.rounds(17, f)[0] == 2
    assert DC.rounds(256, f) == (16, 64, 256, 1, (0, 1, 2, 3)) and DC.rounds(257, f)[3:] == (2, (0,)) and DC.rounds(513, f)[3] == 3
    q = DC.decode_form(128, True)  # Q16: one key per slot and wave while waves are left
    assert DC.rounds(8, q)[0] == 1 and DC.rounds(9, q)[0] == 2 and DC.rounds(128, q)[4] == (0,) and DC.rounds(129, q)[4] == (0, 1)
    assert DC.rounds(512, q)[3:] == (1, (0, 1, 2, 3)) and DC.rounds(513, q)[3:] == (2, (0,))
    for n in (1, 17, 256, 700):  # place() is a bijection of the keys onto (round, row, wave, slot)
        assert len({DC.place(t, n, f) for t in range(n)}) == n
    assert DC.attn_split(DC.SPLIT_MAX_KV, 32, 2) == 16 and DC.attn_split(DC.SPLIT_MAX_KV, 0, 2) == 1 and DC.attn_split(544, 1, 2) == 16
    assert DC.attn_split(63, 32, 2) == 1 and DC.attn_split(4096, 32, 64) == 4 and DC.attn_split(4096, 128, 2) == 16
    S = 16
    assert [DC.split(n, S, 32)[:2] for n in (63, 64, 65, 511, 512, 543)] == [(1, 63), (2, 32), (2, 33), (15, 35), (16, 32), (16, 34)]
    assert DC.split(65, S, 32)[2] == [(0, 33), (33, 65)] and DC.split(543, S, 32)[2][-1] == (510, 543)
    for n in range(1, 545):  # the chunks tile [0, n) and none is empty
        r = DC.split(n, S, 32)[2]
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(e > b for b, e in r)


def test_every_form_and_cut_is_covered():
    t0 = time.perf_counter()
    cases = {n: DC.build_case(n) for n in DC.CASE_NAMES}
    built = time.perf_counter() - t0
    alone = {(c.form.d_head, c.form.kvq, c.block_env): c for c in cases.values() if c.min_keys == 0 and c.name.startswith(c.form.tag) and
             not c.name.endswith(("_store", "_poison"))}
    want = [(d, False, 0) for d in DC.F32_D_HEADS] + [(d, False, e) for e, d in DC.FORCED.items()] + [(d, True, 0) for d in DC.KVQ_D_HEADS]
    assert sorted(alone) == sorted(want)
    for (dh, kvq, env), c in alone.items():
        f = DC.decode_form(dh, kvq, env)
        assert c.form == f and c.S == 1
        lengths = {s.name: s.seq_kv for s in c.steps}
        assert lengths["one"] == 1 and lengths["full"] == f.max_waves * f.kpw * f.u
        assert DC.rounds(lengths["one_wave"], f)[0] == 1 and (DC.rounds(lengths["two_waves"], f)[0] == 2 or f.max_waves == 1)
        assert DC.rounds(lengths["full"], f)[3] == 1 and DC.rounds(lengths["full"], f)[0] == f.max_waves
        assert DC.rounds(lengths["second_round"], f)[3:] == (2, (0,)) and lengths["second_round"] == lengths["full"] + 1
        assert DC.rounds(lengths["two_rounds"], f)[3] == 2 and DC.rounds(lengths["three_rounds"], f)[3] == 3
        if f.q16:
            assert DC.rounds(lengths["row0_full"], f)[4] == (0,) and DC.rounds(lengths["row1"], f)[4] == (0, 1)
        assert {"wave_dead", "first_round_dead", "only_new_column", "all_dead"} <= set(lengths) and ("slot_dead" in lengths) == (f.kpw > 1)
        assert c.max_kv > max(lengths.values())
    split = {(c.form.d_head, c.form.kvq): c for c in cases.values() if c.min_keys}
    assert sorted(split) == sorted((d, q) for d in DC.SPLIT_D_HEADS for q in (False, True))
    for c in split.values():
        assert c.S == 16 and c.max_kv == 544 and {s.seq_kv for s in c.steps} == {63, 64, 65, 511, 512, 543}
        assert [DC.split(n, c.S, c.min_keys)[0] for n in (63, 64, 65, 511, 512, 543)] == [1, 2, 2, 15, 16, 16]
        assert all(s.twice for s in c.steps) and "chunk_dead" in {s.name for s in c.steps}
    # three heads once, a strided row store per form, the store-column and poison carriers
    assert sorted(c.n_heads for c in cases.values()).count(3) == 1 and all(c.n_heads >= 2 for c in cases.values())
    for kind in ("f32", "kvq", "q16"):
        assert any(c.o_rs != 1 for c in cases.values() if c.form.tag.startswith(kind)), kind
        assert any(c.name.endswith("_poison") for c in cases.values() if c.form.tag.startswith(kind)), kind
    for kind in ("f32", "q16"):
        st = next(c for c in cases.values() if c.name.endswith("_store") and c.form.tag.startswith(kind))
        assert [(s.col, s.seq_kv) for s in st.steps] == [(5, 40), (40, 40), (43, 40)]
        sp = next(s for c in split.values() if c.form.tag.startswith(kind) for s in c.steps if s.name == "store_in_chunk_3")
        ranges = DC.split(sp.seq_kv, 16, 32)[2]
        assert ranges[3][0] <= sp.col < ranges[3][1] and len(ranges) == 16
    print(f"{len(cases)} cases, {sum(len(c.steps) for c in cases.values())} steps, built in {built:.2f} s")
    assert built < 5


def test_mask_variants_kill_what_they_name():
    for name in DC.CASE_NAMES:
        c = DC.build_case(name)
        for st in c.steps:
            dead = set(st.dead)
            assert all(0 <= t < st.seq_kv for t in dead)
            if st.name == "only_new_column":
                assert dead == set(range(st.seq_kv)) - {st.col}
            if st.zero:
                assert dead == set(range(st.seq_kv))
            if not st.kills:
                continue
            what, idx = st.kills
            if what == "chunk":
                b, e = DC.split(st.seq_kv, c.S, c.min_keys)[2][idx]
                assert dead == set(range(b, e))
                continue
            at = {"round": 0, "wave": 2, "slot": 3}[what]
            places = {t: DC.place(t, st.seq_kv, c.form) for t in range(st.seq_kv)}
            assert dead == {t for t, p in places.items() if p[at] == idx} and dead and len(dead) < st.seq_kv
            assert st.col not in dead  # the new column stays live
            if what == "wave":
                assert DC.rounds(st.seq_kv, c.form)[0] > idx
            if what == "round":
                assert DC.rounds(st.seq_kv, c.form)[3] == 2


def test_step_uploads_are_nan_behind_seq_kv_and_poison_sits_on_dead_columns():
    for name in DC.CASE_NAMES:
        c = DC.build_case(name)
        dh, n = c.form.d_head, c.max_kv
        for st in c.steps:
            for img in c.cache_images(st):
                rows = img[n * dh // 4:].reshape(n, dh // 32) if c.form.kvq else img.reshape(n, dh)
                bad = set(np.flatnonzero(~np.isfinite(rows).all(axis=1)))
                assert bad == set(range(st.seq_kv, n)) | (set(st.dead) if st.poison else set())
                assert np.isnan(rows[st.seq_kv:]).all()
            m = c.mask_row(st)
            assert set(np.flatnonzero(np.isfinite(m))) == set(range(st.seq_kv)) - set(st.dead)
        assert sorted(s.seq_kv for s in c.steps) == [s.seq_kv for s in c.steps]  # ascending
        w = c.written()
        assert all(len(set(v)) == len(v) and max(v) < c.prog.buffer_sizes[b] for b, v in w.items())


@pytest.mark.parametrize("name", DC.CASE_NAMES)
def test_float64_reference_agrees_with_the_oracle(oracle, name):
    """every clean step: the oracle's head outputs and row-store copies within 2e-6 of float64 attention over the oracle's own
    buffers (the bar of tests/test_attention_cases_host.py); the poisoned step bit-equal to its clean step; sentinels kept"""
    c, runs = DC.oracle_run(oracle, name)
    worst = 0.0
    for st in c.steps:
        got = runs[st.name]
        w = c.written()
        for b, idx in w.items():
            keep = np.ones(got[b].size, bool)
            keep[idx] = False
            assert np.all(got[b][keep] == DC.SENTINEL), (st.name, b)
        if st.poison:
            clean = runs[st.clean_of]
            for b in (DC.QR, DC.KR, DC.AO, DC.O):
                assert np.array_equal(got[b].view(np.uint32), clean[b].view(np.uint32)), (st.name, b)
            continue
        want = DC.float64_heads(c, st, got)
        for b, idx in w.items():
            out = got[b][idx].reshape(c.n_heads, c.form.d_head)
            assert np.isfinite(out).all()
            worst = max(worst, float(np.abs(out - want).max()))
            if st.zero:
                assert np.all(out == 0)
    print(f"{name}: max |oracle - float64| = {worst:.3g}")
    assert worst <= DC.ORACLE_ATOL


def test_fused_positions_from_the_body_geometry():
    """the positions the fused launches are checked at (tests/test_hip_decode_attention.py), per body"""
    P = DC.fused_positions
    # K-on-lanes, 256 threads: 64 heads -> 4 workgroups per head, 32 heads -> 8
    assert P(DC.body_form(64, False, 256), 4, 32, 300) == {"s63": 63, "s64": 64, "s65": 65, "capped": 128, "last_single": 256, "first_two": 257}
    assert P(DC.body_form(128, False, 256), 8, 32, 300) == {"s63": 63, "s64": 64, "s65": 65, "capped": 256, "last_single": 32, "first_two": 33}
    assert P(DC.body_form(128, True, 256), 8, 32, 1100)["first_two"] == 1025
    # K <= 2048, 1024 threads, 16 workgroups per head
    assert P(DC.body_form(64, False, 1024), 16, 32, 4200)["first_two"] == 4097 and P(DC.body_form(128, False, 1024), 16, 32, 2100)["first_two"] == 2049
    # the models that reach them: both bodies x f32 / int8 x d_head 64 / 128, every one met in its second round
    bodies = set()
    for name, (d_model, n_heads, n_kv, d_ff, n_layers, block, n_fused) in DC.FUSED_MODELS.items():
        assert n_heads % n_kv == 0 and 1 <= n_fused <= n_layers and (d_model > 2048) == (block == 256)
        for kvq in (0, 32):
            form, S, max_seq, check = DC.fused_plan(name, kvq)
            bodies.add((block, form.d_head, form.kvq))
            pos = P(form, S, 32, max_seq)
            assert {63, 64, 65, pos["first_two"] - 1, pos["first_two"], S * 32} <= set(check) and max(check) <= max_seq
            assert max(DC.rounds(e - b, form)[3] for b, e in DC.split(pos["first_two"], S, 32)[2]) == 2
    assert bodies == {(b, d, q) for b in (256, 1024) for d in (64, 128) for q in (False, True)}
    assert [DC.fused_splits(n, 1 << 20) for n in ("smollm", "dh128", "kon_dh64", "kon_dh128")] == [16, 4, 4, 8]
