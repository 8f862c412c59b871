"""The weight case table (tests/weight_cases.py) checked on the host, for every case tests/test_hip_weight_values.py runs on the
device: the profiles really have the properties they are named for (else the device test would pass on the wrong values), the
oracle's exact path alone meets the device test's bound against the float64 reference (so the bound judges the kernels, not the
reference), the oracle's GGUF loader restatement returns the profiles' blocks bit for bit (negative, subnormal and -0.0 scales
included), and the oracle's W8A8 arm is sign-symmetric and within the reference's inter-arm bound on GGUF-like weights.
CPU only (no GPU marker)."""
import numpy as np
import pytest

from tests import weight_cases as WC

f32 = np.float32


def _all_weights(profile):
    for cls, K, N, bs, part in WC.distinct_weights():
        for phase in WC.variants(profile, N, bs):
            yield (cls, K, N, bs, part, phase), WC.weight(profile, cls, K, N, bs, part, phase)


def test_table_covers_the_routes_and_classes():
    assert {c.cls for c in WC.CASES} == set(WC.CLASSES)
    assert {c.route for c in WC.CASES} == {"matvec-nol", "matvec-kon", "kon-rows", "tile", "xdl2", "xdl5", "xdl4", "xdl4-m32", "grouped", "raw", "gguf-pack"}
    for c in WC.CASES:  # the dispatch conditions the table relies on (zgml_amd/csrc: compile_program, launch_qmatmul, launch_xdl2)
        if c.route == "matvec-nol":
            assert c.M == 1 and c.K < 2049
        if c.route in ("matvec-kon", "kon-rows"):
            assert c.K >= 2049 and WC.is_q4(c.cls) and WC.is_f16(c.cls) and (c.M == 1 or (c.small_m and 2 <= c.M <= 8))
        if c.route == "tile":
            assert c.M > 1 and not (WC.is_q4(c.cls) and WC.is_f16(c.cls))
        if c.route in ("xdl2", "xdl5", "xdl4", "xdl4-m32"):
            assert c.M > 1 and WC.is_q4(c.cls) and WC.is_f16(c.cls) and (c.K + 31) // 32 <= 4 * 96
        if c.route == "xdl2":
            assert c.M <= 32 and (c.N // 32 + 7) // 8 < 40
        if c.route == "xdl5":
            assert c.M <= 32 and (c.N // 32 + 7) // 8 >= 40
        if c.route == "xdl4":
            assert c.M > 32
        if c.route == "xdl4-m32":  # launch_xdl2: two m-tiles, K cut into sk >= 2 slices of >= 16 steps (256 CUs, 8 waves)
            S, bcs = ((c.K + 31) // 32 + 3) // 4, c.N // 32
            sk = min(-(-256 // bcs), 4, -(-S // 8))
            assert 16 < c.M <= 32 and (bcs + 7) // 8 < 40 and sk >= 2 and S // sk >= 16
        if c.route == "raw":
            assert c.bs != 32 or c.N % 32 != 0


def test_negated_is_positive_with_every_scale_negated():
    for key, (data, scales) in _all_weights("negated"):
        cls, K, N, bs, part, phase = key
        d0, s0 = WC.weight("positive", cls, K, N, bs, part, phase)
        assert np.array_equal(data, d0) and np.array_equal(scales, -s0) and np.all(s0 > 0), key


def test_gguf_profile_has_both_signs_and_the_nibble_zero():
    seen_negative = 0
    for key, (data, scales) in _all_weights("gguf"):
        cls, K, N, bs, part, phase = key
        if scales.size >= 64:
            share = float(np.mean(scales < 0))
            assert 0.4 <= share <= 0.6, (key, share)
            seen_negative += 1
        if WC.is_q4(cls):
            blocks = data.reshape(-1, bs)
            live = scales != 0
            assert np.all((blocks[live] == -8).any(axis=1)), key  # v_max / d == -8: stored nibble 0
            assert np.all(blocks[~live] == 0), key
            assert np.unique(np.frexp(scales[live])[1]).size >= 8, key  # magnitudes over many binades
    assert seen_negative


def test_extremes_profile_shows_every_pattern_and_both_signs():
    for c in WC.CASES:
        for t, N in enumerate(c.Ns):
            mags, signs, zeros, neg_zeros = set(), set(), 0, 0
            for phase in WC.variants("extremes", N, c.bs):
                data, scales = WC.weight("extremes", c.cls, c.K, N, c.bs, t, phase)
                h = (scales / f32(1.0 + 2.0 ** -20) if not WC.is_f16(c.cls) else scales).astype(np.float16).view(np.uint16)
                mags |= set((h & 0x7FFF).tolist())
                signs |= set((h >> 15).tolist())
                zeros += int(np.sum(scales == 0))
                neg_zeros += int(np.sum(np.signbit(scales) & (scales == 0)))
                if c.bs == 32 and N % 32 == 0:  # one magnitude class per block-column
                    m = (h & 0x7FFF).reshape(c.K, N // 32)
                    assert np.all(m == m[0]), c.id
                if not WC.is_f16(c.cls):
                    assert np.all(WC.f16_exact(scales) == (scales == 0)), c.id
            assert mags == set(WC.EXTREME_BITS) and signs == {0, 1}, (c.id, sorted(mags))
            assert 0 < neg_zeros < zeros or zeros < 12, c.id  # both 0.0 and -0.0 occur


def test_zero_blocks_profile_has_an_all_zero_output_column():
    for c in WC.CASES:
        x = WC.case_x(c)
        for (data, scales), N in zip(WC.case_weights(c, "zero_blocks"), c.Ns):
            _, bound = WC.reference(data, scales, x, c.M, N, c.K, c.bs)
            dead = np.all(bound == 0, axis=0)
            assert dead.any() and not dead.all(), c.id
            nb = scales.size
            blocks = np.zeros(nb * c.bs, np.int8)
            blocks[:data.size] = data
            share = np.mean((scales == 0) | np.all(blocks.reshape(nb, c.bs) == 0, axis=1))
            assert share >= 0.2 or nb < 32, (c.id, share)


@pytest.mark.parametrize("profile", WC.PROFILES)
def test_oracle_alone_meets_the_device_bound(oracle, profile):
    """|oracle - want64| <= 2e-5 * bound64 + 1e-30 and exactly 0 where bound64 == 0, for every case and variant of the device test"""
    oracle.set_threads(8)
    worst, done = 0.0, set()
    for c in WC.CASES:
        x = WC.case_x(c)
        for t, N in enumerate(c.Ns):
            for phase in WC.variants(profile, N, c.bs):
                key = (c.cls, c.M, c.K, N, c.bs, t, phase)
                if key in done:
                    continue
                done.add(key)
                data, scales = WC.weight(profile, c.cls, c.K, N, c.bs, t, phase)
                want, bound = WC.reference(data, scales, x, c.M, N, c.K, c.bs)
                got = oracle.qmatmul_exact(np.ascontiguousarray(data), np.ascontiguousarray(scales), x, c.M, N, c.K, c.bs).reshape(c.M, N).astype(np.float64)
                assert np.all(np.isfinite(got)), c.id
                assert np.all(np.abs(got - want) <= WC.TOL * bound + WC.FLOOR), (c.id, profile, phase, float(np.max(np.abs(got - want) / (bound + WC.FLOOR))))
                assert np.all(got[bound == 0] == 0), (c.id, profile, phase)
                worst = max(worst, float(np.max(np.abs(got - want)[bound > 0] / bound[bound > 0], initial=0.0)))
    print(f"{profile}: the oracle's worst |delta| / bound64 = {worst:.2e} (bar {WC.TOL:.0e})")
    assert worst <= WC.TOL / 10  # an order of margin (sequential f32 sums over K <= 8192): the bound is about the kernels


@pytest.mark.parametrize("profile", WC.PROFILES)
def test_gguf_blocks_round_trip_bit_for_bit(oracle, profile):
    n = 0
    for key, (data, scales) in _all_weights(profile):
        cls, K, N, bs, part, phase = key
        if not cls.startswith("gguf_"):
            continue
        raw = WC.gguf_blocks(cls, data, scales)
        d2, s2 = oracle.gguf_to_int8(raw, data.size, cls[5:])
        assert np.array_equal(d2, data), key
        assert np.array_equal(s2.view(np.uint32), scales.view(np.uint32)), key  # bits: -0.0 and the subnormals too
        n += 1
    assert n


@pytest.mark.parametrize("K,N", WC.W8A8_SHAPES)
@pytest.mark.parametrize("kind", WC.W8A8_KINDS)
def test_oracle_w8a8_arm_is_sign_symmetric_and_inside_the_inter_arm_bound(oracle, K, N, kind):
    """prepareTransposed re-quantises |w| / max with truncation and gemvRange multiplies by the block scales: both are odd in the
    weight, so negated scales give exactly the negated result; over GGUF-like weights the arm stays within the reference's own
    bound between its two arms (0.15 of the largest output: src/quant.zig:1165-1210, as tests/test_hip_w8a8.py uses it)."""
    x = np.random.default_rng(K + N).standard_normal(K).astype(f32)

    def arm(profile):
        data, scales = WC.w8a8_weight(profile, kind, K, N)
        t_data, t_scales = oracle.prepare_transposed(data, scales, K, N, 32)
        return oracle.gemv(t_data, t_scales, x, N, K, 32), oracle.qmatmul_exact(data, scales, x, 1, N, K, 32)
    pos, _ = arm("positive")
    neg, _ = arm("negated")
    assert np.array_equal(neg, -pos)
    got, exact = arm("gguf")
    assert np.abs(got - exact).max() < 0.15 * np.abs(exact).max()
