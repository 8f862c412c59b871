"""tests/dense_f16_cases.py pinned on the CPU before any device runs: the restated launcher rules give exactly the instantiations the
table claims and every cut it names; the plan-level cases join and reuse as declared; the poison lies where the layout says; and
on every promoted case the oracle's f16 path stays inside the contract bar against float64 on every output (so a device miss is
the device's), keeps every sentinel, and gives float64's non-finite pattern on the overflow profile."""
import time

import numpy as np
import pytest

from tests import dense_f16_cases as DF

f32 = np.float32


def test_restated_rules_on_known_launches():
    r = DF.route(1, 4096, 4096, True, 4096, False)  # the benchmark's token_len 1 leg below the NT threshold
    assert (r.name, r.waves, r.step, r.grid, r.lds) == ("dense_f16_kernel<0, true, 1, false>", 4, 32, (256, 1), 8192)
    r = DF.route(32, 4096, [4096, 4096, 4096], True, 4096, True)  # q / k / v of Llama-2-7B prefill: one NT launch
    assert (r.name, r.waves, r.step, r.tiles, r.grid, r.CG) == ("dense_f16_tile2_kernel<2, true, 1>", 8, 32, 2, (768, 1), 1)
    r = DF.route(32, 4096, [11008, 11008], True, 4096, True)  # gate / up: 1376 column groups, 688 each
    assert (r.name, r.grid) == ("dense_f16_tile2_kernel<2, true, 2>", (688, 1))
    assert DF.route(128, 4096, 4096, True, 4096, True).name == "dense_f16_tile2_kernel<8, true, 1>"
    assert DF.route(129, 64, 32, True, 64, True).name == "dense_f16_tile2_kernel<8, false, 1>"  # two row groups: never NT
    assert [DF.tiles_per_wg(M) for M in (2, 16, 17, 32, 33, 64, 65, 200)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert [DF.tiles_per_wg(M, {"ZGML_F16_TILE2_WIDE": 0}) for M in (16, 17, 129)] == [1, 2, 2]
    s = DF.route(32, 1024, 32, True, 1028, False, DF.FORCED["staged"])
    assert (s.name, s.waves, s.lds) == ("dense_f16_kernel<2, true, 1, false>", 8, 132096) and s.lds > 64 * 1024
    assert DF.route(32, 1024, 32, True, 1027, False, DF.FORCED["staged"]).name == "dense_f16_kernel<2, false, 1, false>"
    assert DF.route(16, 64, 24576, True, 68, False, DF.FORCED["staged"]).name == "dense_f16_kernel<1, true, 2, false>"
    assert DF.packed_bytes(DF.FILLER_K, DF.FILLER_N) == DF.NT_BYTES and DF.packed_bytes(3, 16) == 1024
    assert DF.a_unpadded(32, 256) and not DF.a_unpadded(48, 256) and not DF.a_unpadded(32, 37)


def test_every_instantiation_is_reached_and_no_other():
    t0 = time.perf_counter()
    cases = {n: DF.build_case(n) for n in DF.CASE_NAMES}
    built = time.perf_counter() - t0
    default = [cases[n] for n in DF.DEFAULT_CASES]
    assert len(DF.DEFAULT_INSTANTIATIONS) == 16
    assert {r.name for c in default for r in c.routes.values()} == DF.DEFAULT_INSTANTIATIONS
    for key, want in DF.FORCED_INSTANTIATIONS.items():
        mine = [cases[n] for n in DF.forced_cases(key)]
        assert mine and all(c.forced == key for c in mine)
        assert {r.name for c in mine for r in c.routes.values()} == want, key
    # at least one f16_edges matmul on every instantiation, an overflow on every kernel family and R
    by_profile = {}
    for c in cases.values():
        for m in c.mats:
            if m.promoted:
                L = next(L for L in DF.plan(c.prog, c.env) if m.op in (L.parts or [L.lo]))
                by_profile.setdefault(m.profile, set()).add(c.routes[L.lo].name)
    everything = DF.DEFAULT_INSTANTIATIONS.union(*DF.FORCED_INSTANTIATIONS.values())
    assert by_profile["f16_edges"] == everything
    assert {n.split(",")[0] for n in by_profile["overflow"]} == {n.split(",")[0] for n in everything}
    assert {"dense_f16_kernel<0, true, 1, false>", "dense_f16_tile2_kernel<2, false, 1>", "dense_f16_tile2_kernel<4, false, 1>",
            "dense_f16_tile2_kernel<8, false, 1>"} <= by_profile["zero_row"]
    assert [c.name for c in cases.values() if c.nt] == ["nt_program"]
    print(f"{len(cases)} cases ({len(default)} under default switches), {sum(len(c.mats) for c in cases.values())} matmuls, built in {built:.2f} s")


def test_every_named_cut_is_met():
    for name in DF.CASE_NAMES:
        c = DF.build_case(name)
        if not c.expect:
            continue
        m = c.mats[0]
        r = c.routes[m.op]
        got = dict(waves=r.waves, trips=r.trips(m.K), live_last=r.live_last(m.K), R=r.R, tiles=r.tiles, padded_rows=r.tiles * 16 - m.M,
                   grid_y=r.grid[1], CG=r.CG)
        assert {k: got[k] for k in c.expect} == c.expect, name
        if len(c.mats) == 1:
            assert r.grid[0] == DF.cdiv(m.N // 16, r.CG), name
    # the cuts the issue names, read back from the tables
    assert DF.MV_CUTS[288] == (2, 1, 9) and DF.MV_CUTS[1024] == (4, 1, 32) and DF.MV_CUTS[1056] == (4, 2, 1) and DF.MV_CUTS[1030] == (4, 2, 1)
    assert DF.T2_CUTS[2][256] == (8, 1, 8) and DF.T2_CUTS[4][800] == (8, 2, 1) and DF.T2_CUTS[8][544] == (8, 2, 1)
    assert DF.M_CUTS[48][2] == 16 and DF.M_CUTS[129][3] == 2
    # the ragged trips really leave clamped duplicates behind the last live chunk
    for name in ("mv_k288_n16_overflow", "mv_k1056_n16_overflow", "t2_m32_k288_overflow", "t2_m64_k800_overflow", "t2_m128_k544_overflow"):
        c = DF.build_case(name)
        r = c.routes[0]
        assert r.live_last(c.mats[0].K) % r.step != 0, name
    g = DF.build_case("t2_cg2_group")
    assert g.routes[0].grid == (640, 1) and g.routes[0].CG == 2  # part 1 begins at workgroup 320
    big = DF.build_case("t2_cg2_m32").mats[0]
    assert (big.N // 16) * DF.cdiv(big.K, 32) * 64 > 2048 * 256  # pack_f16_kernel: more items than one pass of its grid
    assert DF.build_case("t2_cg2_refused_odd").routes[0].name == "dense_f16_tile2_kernel<2, false, 1>"


def test_plan_level_cases_join_and_reuse_as_declared():
    want = {"plan_three": ([(0, 2)], {0: False}), "plan_four": ([(0, 2), (3, 3)], {0: False, 3: True}),
            "plan_parts_n": ([(0, 2)], {0: False}), "plan_dst_overlap": ([(0, 0), (1, 1)], {0: False, 1: True}),
            "plan_other_k": ([(0, 0), (1, 1)], {0: False, 1: False}), "plan_other_a_rs": ([(0, 0), (1, 1)], {0: False, 1: False}),
            "plan_q4_between": ([(0, 0), (1, 1), (2, 2)], {0: False, 2: False}), "t2_cg2_group": ([(0, 1)], {0: False}),
            "t2_rows_17_32": ([(0, 0), (1, 1)], {0: False, 1: False})}
    for name, (launches, reuse) in want.items():
        c = DF.build_case(name)
        assert c.launches == launches and DF.reuse_a(c.prog) == reuse, name
    c = DF.build_case("plan_parts_n")
    assert [m.N for m in c.mats] == [32, 16, 48] and c.routes[0].grid == (6, 1)
    q = DF.build_case("plan_q4_between")
    assert q.prog.ops[1].kind == "qmatmul" and DF.q_splits(32, 256, 64)
    nt = DF.build_case("nt_program")
    assert DF.stream_nt(nt.prog) and len(nt.launches) == len(nt.prog.ops) and not any(DF.reuse_a(nt.prog).values())
    assert sorted(r.name for r in nt.routes.values()) == sorted(
        ["dense_f16_kernel<0, true, 1, true>"] * 3 + ["dense_f16_kernel<0, false, 1, true>"] * 2 + [f"dense_f16_tile2_kernel<{R}, true, 1>" for R in (1, 2, 2, 4, 8, 8)] +
        ["dense_f16_tile2_kernel<2, true, 2>", "dense_f16_tile2_kernel<1, true, 2>", "dense_f16_tile2_kernel<8, false, 1>"])


def test_promotion_is_refused_clause_by_clause():
    for clause in DF.REFUSED_CLAUSES:
        for M in (1, 17):
            c = DF.build_case(f"refused_{clause}_m{M}")
            weights = DF.promoted(c.prog)
            assert all(m.b_buf not in weights for m in c.mats if not m.promoted) and not c.mats[0].promoted, c.name
    # ... and each clause alone decides: the plain program of the same shape is promoted
    assert DF.build_case("mv_k256_n16_normal").mats[0].promoted and DF.build_case("t2_m17_k256").mats[0].promoted


def test_poison_and_profiles_lie_where_the_layout_says():
    for name in DF.CASE_NAMES:
        c = DF.build_case(name)
        if name.startswith("refused_"):
            continue
        for m in c.mats:
            assert m.a_rs > m.K and m.d_rs > m.N, name
            img = c.images[m.a_buf]
            live = np.zeros(img.size, bool)
            for x in c.mats:
                if x.a_buf == m.a_buf:
                    live[(x.a_off + np.arange(x.M)[:, None] * x.a_rs + np.arange(x.K)[None, :]).ravel()] = True
            assert np.isnan(img[~live]).all() and np.isfinite(img[live]).all() and not live[:m.a_off].any() and not live[-5:].any(), name
            op = c.prog.ops[m.op].geom
            b = c.images[m.b_buf]
            at = op.b_offset + np.arange(m.K)[:, None] * op.b_row_stride + np.arange(m.N)[None, :] * op.b_col_stride
            keep = np.ones(b.size, bool)
            keep[at.ravel()] = False
            if not any(x is not m and x.b_buf == m.b_buf for x in c.mats):
                assert np.isnan(b[keep]).all() and keep[:op.b_offset].all() and keep[-3:].all() and np.array_equal(b[at], m.B), name
            d = c.images[m.d_buf]
            assert np.all(d == DF.SENTINEL), name
    # the refused promotions share buffers between A, B and dst (that is what some clauses are), so their layout is pinned over
    # the union of what the matmuls read: a_rs > K and dst_rs > N, NaN (or the sentinel of a dst region) in every operand word
    # that no matmul reads, finite values in every word one does. The one exemption: the second matmul of `also_an_a` reads
    # the first's dense B rows as its A, so its a_rs equals its K.
    for name in (n for n in DF.CASE_NAMES if n.startswith("refused_")):
        c = DF.build_case(name)
        live = {b: np.zeros(img.size, bool) for b, img in c.images.items()}
        for m in c.mats:
            g = c.prog.ops[m.op].geom
            assert m.d_rs > m.N and (m.a_rs > m.K * m.a_cs or (name.startswith("refused_also_an_a") and m is c.mats[1])), name
            live[m.a_buf][(m.a_off + np.arange(m.M)[:, None] * m.a_rs + np.arange(m.K)[None, :] * m.a_cs).ravel()] = True
            live[m.b_buf][(g.b_offset + np.arange(m.K)[:, None] * g.b_row_stride + np.arange(m.N)[None, :] * g.b_col_stride).ravel()] = True
        for m in c.mats:
            for b in (m.a_buf, m.b_buf):
                img = c.images[b]
                assert np.all(np.isnan(img[~live[b]]) | (img[~live[b]] == DF.SENTINEL)) and np.isfinite(img[live[b]]).all(), (name, b)
                assert np.isnan(img[~live[b]]).any(), (name, b)
            d = c.images[m.d_buf]
            assert np.all(d[m.written()] == DF.SENTINEL) and d[m.written().max() + 1] == DF.SENTINEL and d[m.d_off - 1] == DF.SENTINEL, name
    assert sum(c.mats[0].b_layout == "wide" for c in map(DF.build_case, DF.CASE_NAMES)) >= 1
    assert sum(c.mats[0].b_layout == "kcontig" for c in map(DF.build_case, DF.CASE_NAMES)) >= 1
    # f16_edges: the subnormal-only columns hold nothing but f16 subnormals and zeros after rounding, and some of each
    m = DF.build_case("t2_m32_k1056_f16_edges").mats[0]
    with np.errstate(over="ignore"):
        b16 = m.B.astype(np.float16)
    cols = DF.subnormal_only_columns(m.N)
    assert cols and np.all(np.abs(b16[:, cols].astype(np.float64)) < 2.0 ** -14) and np.count_nonzero(b16[:, cols]) > m.K
    bits = set(np.unique(b16.view(np.uint16) & 0x7FFF))
    assert {0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF} <= bits and not np.isinf(b16).any()
    assert np.all(b16[:, 4].view(np.uint16) & 0x7FFF == 0x7BFF)  # 65519.992 rounds down, one ulp more would be inf
    with np.errstate(over="ignore"):
        assert np.float32(65520.0).astype(np.float16) == np.inf
    assert {0x0000, 0x0001, 0x0400} <= set(np.unique(DF.CROSS.astype(np.float16).view(np.uint16)))
    a16 = m.A.astype(np.float16)
    assert np.all(np.abs(a16[1].astype(np.float64)) <= 2.0 ** -14) and np.count_nonzero(a16[1]) and np.all(np.abs(a16[3].astype(np.float64)) <= 2.0 ** -14)


def test_a_flushed_subnormal_operand_misses_the_device_bar():
    """what the device test holds the M > 1 forms to on f16_edges (check_mat, matrix_cores) is missed by float64 results with
    the subnormals of A, of B or of both flushed; the term itself is zero where no 32-k dot mixes magnitudes"""
    for name in ("t2_m32_k1056_f16_edges", "t2_m16_k1056_f16_edges", "staged_m17_k1024"):
        c = DF.build_case(name)
        m = c.mats[0]
        assert m.profile == "f16_edges" and m.M > 1
        A, B = m.A.astype(np.float16).astype(np.float64), m.B.astype(np.float16).astype(np.float64)
        fa, fb = np.where(np.abs(A) < 2.0 ** -14, 0, A), np.where(np.abs(B) < 2.0 ** -14, 0, B)
        image = np.full(c.prog.buffer_sizes[m.d_buf], DF.SENTINEL, f32)
        image[m.written()] = A @ B
        DF.check_mat(c, m, image, matrix_cores=True)
        for A2, B2 in ((fa, B), (A, fb), (fa, fb)):
            image[m.written()] = A2 @ B2
            with pytest.raises(AssertionError, match="miss the contract|of the bar"):
                DF.check_mat(c, m, image, matrix_cores=True)
        assert DF.subnormal_slack(m, 0, 7) == 0 and DF.subnormal_slack(m, 0, 5) == 0  # a normal column, a column of ones and zeros


_PROMOTED = [n for n in DF.CASE_NAMES if not n.startswith("refused_")]


@pytest.fixture()
def f16_oracle(oracle):
    oracle.set_f16_dense(True)
    yield oracle.OracleBackend()
    oracle.set_f16_dense(False)


@pytest.mark.parametrize("name", _PROMOTED)
def test_oracle_stays_inside_the_bar(f16_oracle, name):
    """every output of every matmul of every promoted case (the NT program: each matmul in a program of its own, without the
    384 MiB filler image)"""
    c = DF.build_case(name)
    worst = 0.0
    if c.nt:
        for m in c.mats:
            prog, d = DF.solo_program(c, m)
            got, _ = DF.run(f16_oracle, prog, [d])
            worst = max(worst, DF.check_mat(c, m, got[d][0])[0])
            keep = np.ones(got[d][0].size, bool)
            keep[m.written().ravel()] = False
            assert np.all(got[d][0][keep] == DF.SENTINEL), (name, m.op)
    else:
        bufs = sorted({m.d_buf for m in c.mats})
        got, _ = DF.run(f16_oracle, c.prog, bufs, c.exec_inputs, c.images)
        for m in c.mats:
            worst = max(worst, DF.check_mat(c, m, got[m.d_buf][0])[0])
        DF.untouched(c, {b: got[b][0] for b in bufs})
    print(f"{name}: oracle worst error / bound = {worst:.3g} (bar {DF.TOL:g})")
