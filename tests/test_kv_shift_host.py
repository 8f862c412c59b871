"""CPU tests of the context shift's rule (zgml_amd/csrc/kv_shift.h): the header, compiled alone for the CPU
(tests/cpp/kv_shift_probe.cpp), against the numpy model of tests/kv_shift_model.py to the bit, on f32 and int8 lanes; what the rule
means (a rotation by minus `discard` positions, built from the table's own entries); how far a shifted key lies from a freshly
roped one (the tables' angle rounding, recorded); and the algebra of two shifts on the model."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import kv_shift_model as M

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
U = 2.0 ** -24  # the unit roundoff of f32


def kv_shift_probe():
    src, exe = ROOT / "tests" / "cpp" / "kv_shift_probe.cpp", ROOT / "tests" / "cpp" / "_build" / "kv_shift_probe"
    hdrs = [ROOT / "zgml_amd" / "csrc" / "kv_shift.h", ROOT / "zgml_amd" / "csrc" / "kvq.h"]
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(src)], check=True)
    return exe


def probe_shift(kind, img, dh, n_cols, keep, discard, n_filled, is_k, c, s, tmp_path):
    """the lane image (f32 array; for "i8" the f32 view of the cache image) through the probe -> the shifted image"""
    frows, fin, fout = tmp_path / "rows.f32", tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([c, s]).astype(f32).tofile(frows)
    np.ascontiguousarray(img, f32).tofile(fin)
    subprocess.run([str(kv_shift_probe()), kind, str(dh), str(n_cols), str(keep), str(discard), str(n_filled), str(int(is_k)), str(frows), str(fin),
                    str(fout)], check=True)
    out = np.fromfile(fout, f32)
    assert out.size == img.size
    return out


def edge_lane(dh, n_cols, rng):
    """random columns of mixed magnitudes, with an all-zero 32-block, an all-zero column, a column whose maximum sits in the `hi`
    half and one whose maximum sits in the `lo` half"""
    cols = ((rng.random((n_cols, dh)) - 0.5) * 2).astype(f32) * (10.0 ** rng.integers(-3, 3, (n_cols, 1))).astype(f32)
    cols[n_cols - 2, :32] = 0.0
    cols[n_cols - 3] = 0.0
    cols[n_cols - 4] *= f32(7.9) / np.abs(cols[n_cols - 4]).max()
    cols[n_cols - 4, dh // 2 + 3] = 8.0  # (127 / 8 and 8 * (127 / 8) are exact: the quantised maximum is 127)
    cols[n_cols - 5] *= f32(7.9) / np.abs(cols[n_cols - 5]).max()
    cols[n_cols - 5, 1] = -8.0
    return cols


def angle_rows(dh, discard, oracle, max_seq=64):
    cos, sin = oracle.rope_tables(dh, max_seq)
    return M.shift_rows(cos, sin, discard)


CASES = [(0, 1, 2), (4, 8, 24), (3, 5, 21), (0, 23, 24), (4, 20, 24), (2, 0, 24)]  # (keep, discard, n_filled) at n_cols 24


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("is_k", [True, False])
def test_header_equals_the_model_on_f32_lanes(oracle, tmp_path, dh, is_k):
    rng, n_cols = np.random.default_rng(dh), 24
    lane = edge_lane(dh, n_cols, rng)
    for keep, discard, n_filled in CASES:
        c, s = angle_rows(dh, discard, oracle)
        got = probe_shift("f32", lane.ravel(), dh, n_cols, keep, discard, n_filled, is_k, c, s, tmp_path)
        want = M.shift_f32(lane, keep, discard, n_filled, is_k, c, s)
        assert np.array_equal(got.view(np.uint32), want.ravel().view(np.uint32)), (keep, discard, n_filled)
        moved = n_filled - keep - discard
        if is_k and discard and moved > 0:
            assert not np.array_equal(want[keep:keep + moved], lane[keep + discard:n_filled])  # (the rotation did something)


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("is_k", [True, False])
def test_header_equals_the_model_on_int8_lanes(oracle, tmp_path, dh, is_k):
    rng, n_cols = np.random.default_rng(100 + dh), 24
    lane = edge_lane(dh, n_cols, rng)
    q, sc = M.quantise(lane)
    assert np.all(sc[n_cols - 3] == 1.0) and not q[n_cols - 3].any()  # the all-zero column: scale 1, quants 0
    assert np.abs(lane[n_cols - 4, :dh // 2]).max() < 8 and q[n_cols - 4, dh // 2 + 3] == 127  # the column's maximum sits in the `hi` half
    img = np.concatenate([q.ravel().view(f32), sc.ravel()])
    for keep, discard, n_filled in CASES:
        c, s = angle_rows(dh, discard, oracle)
        got = probe_shift("i8", img, dh, n_cols, keep, discard, n_filled, is_k, c, s, tmp_path)
        want = M.shift_cache_image(img.copy(), n_cols, dh, keep, discard, n_filled, is_k, c, s)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (keep, discard, n_filled)
    # the block maxima are taken over the ROTATED values: a rotated column reaches 127 in every block that is not all zero (126
    # where fl(mx * fl(127 / mx)) falls a hair below 127 and the truncation takes it)
    c, s = angle_rows(dh, 8, oracle)
    q2, sc2 = M.shift_i8(q, sc, 4, 8, 24, True, c, s)
    blocks = np.abs(q2[4:16].astype(np.int32)).reshape(12, dh // 32, 32).max(axis=2)
    assert np.all((blocks >= 126) | (sc2[4:16] == 1.0))


@pytest.mark.parametrize("dh,max_seq", [(32, 64), (64, 2048), (128, 2048)])
def test_the_rule_is_the_rotation_by_minus_discard_positions(oracle, dh, max_seq):
    """In float64, K' = R(-discard theta) K with R built from the TABLE'S OWN f32 entries c, s: lo' = lo c + hi s, hi' = hi c - lo s.
    The rule rounds four times per output. Each product carries a relative error <= u = 2^-24, the sum another u on the rounded
    products: |err| <= u (|lo c| + |hi s|) + u (1 + u)(|lo c| + |hi s|) < 2 u (1 + u)(|lo||c| + |hi||s|), and by Cauchy-Schwarz
    |lo||c| + |hi||s| <= |(lo, hi)| |(c, s)| with |(c, s)| <= 1 + 2 u (two entries each within u / 2 ulp-relative of a point on the
    unit circle). So every output lies within 2.001 u |(lo, hi)| of the exact rotation: two f32 ulp of the pair's magnitude."""
    rng = np.random.default_rng(dh)
    cos, sin = oracle.rope_tables(dh, max_seq)
    hd = dh // 2
    worst = 0.0
    for discard in (1, 7, max_seq // 2, max_seq - 1):
        c, s = M.shift_rows(cos, sin, discard)
        assert np.all(np.hypot(c.astype(np.float64), s.astype(np.float64)) <= 1 + 2 * U)
        k = ((rng.random((16, dh)) - 0.5) * 2).astype(f32)
        got = M.rotate(k, c, s).astype(np.float64)
        lo, hi, c64, s64 = k[:, :hd].astype(np.float64), k[:, hd:].astype(np.float64), c.astype(np.float64), s.astype(np.float64)
        want = np.concatenate([lo * c64 + hi * s64, hi * c64 - lo * s64], axis=1)
        mag = np.hypot(lo, hi)
        err = np.abs(got - want) / np.concatenate([mag, mag], axis=1)
        worst = max(worst, float(err.max()))
    print(f"d_head {dh} max_seq {max_seq}: worst error {worst / U:.3f} u of the pair's magnitude (bound 2.001 u)")
    assert worst <= 2.001 * U


def rope(k, cos, sin, pos):
    """the rope op's rotation of columns k [n, d_head] at position pos with the f32 tables (oracle/zgml_oracle.c zo_rope)"""
    hd = k.shape[1] // 2
    lo, hi, c, s = k[:, :hd], k[:, hd:], cos[pos, :hd], sin[pos, :hd]
    return np.concatenate([(lo * c).astype(f32) - (hi * s).astype(f32), (hi * c).astype(f32) + (lo * s).astype(f32)], axis=1).astype(f32)


def fresh_gap(oracle, dh, max_seq, keep=4):
    """the largest distance, over positions and pairs, between a shifted unit key and the same key freshly roped at the new position"""
    cos, sin = oracle.rope_tables(dh, max_seq)
    hd = dh // 2
    k = np.zeros((1, dh), f32)
    k[0, :hd], k[0, hd:] = f32(np.cos(0.3)), f32(np.sin(0.3))  # every pair a unit vector
    discard = (max_seq - keep) // 2
    c, s = M.shift_rows(cos, sin, discard)
    worst = 0.0
    for pos in range(keep + discard, max_seq):
        shifted = M.rotate(rope(k, cos, sin, pos), c, s).astype(np.float64)
        fresh = rope(k, cos, sin, pos - discard).astype(np.float64)
        d = shifted - fresh
        worst = max(worst, float(np.hypot(d[0, :hd], d[0, hd:]).max()))
    return worst


@pytest.mark.parametrize("dh,max_seq", [(32, 64), (64, 64), (64, 2048), (128, 2048)])
def test_record_the_gap_to_a_freshly_roped_key(oracle, dh, max_seq):
    """RECORDED, not a property of the kernel: a shifted key is not bit-equal to the key roped at the new position, because the
    tables' angles are rounded. Row p holds cos / sin of fl(p / fl(base^(2i/d))): two roundings of an angle of up to p radians, so
    each row's angle is off by up to about 2 u p, and three rows meet in the comparison (p, discard, p - discard, whose positions
    sum to at most 2 max_seq): the gap of a unit pair is bounded by about 4 u max_seq plus the few u of the arithmetic — 1.6e-5 at
    max_seq 64, 4.9e-4 at 2048. Measured here (unit pairs, base 10000, keep 4, discard half the rest): 1.9e-6 at (32, 64), 2.9e-6 at
    (64, 64), 6.1e-5 at (64, 2048), 7.6e-5 at (128, 2048)."""
    gap = fresh_gap(oracle, dh, max_seq)
    print(f"d_head {dh} max_seq {max_seq}: a shifted unit key lies {gap:.3g} from the freshly roped one")
    assert 0 < gap <= 4 * U * max_seq + 8 * U


def test_two_shifts_map_columns_as_one(oracle):
    """A shift by a followed by a shift by b puts the same columns in the same places as one shift by a + b; the values differ by
    the rounding of one more rotation and by the tables' angle rounding (row a + b against rows a and b). RECORDED: the bound is
    that of the test above for three rows whose positions sum to 2 (a + b), plus the 2.001 u of each of the three rotations."""
    dh, n_cols, keep, a, b = 64, 64, 4, 9, 12
    rng = np.random.default_rng(7)
    cos, sin = oracle.rope_tables(dh, n_cols)
    lane = ((rng.random((n_cols, dh)) - 0.5) * 2).astype(f32)
    marks = np.arange(n_cols, dtype=f32)[:, None] * np.ones((1, dh), f32)  # a V lane whose values name their column
    two_v = M.shift_f32(M.shift_f32(marks, keep, a, n_cols, False), keep, b, n_cols - a, False)
    one_v = M.shift_f32(marks, keep, a + b, n_cols, False)
    n_new = n_cols - a - b
    assert np.array_equal(two_v[:n_new], one_v[:n_new])
    assert np.array_equal(one_v[keep:n_new, 0], np.arange(keep + a + b, n_cols, dtype=f32))
    two = M.shift_f32(M.shift_f32(lane, keep, a, n_cols, True, *M.shift_rows(cos, sin, a)), keep, b, n_cols - a, True, *M.shift_rows(cos, sin, b))
    one = M.shift_f32(lane, keep, a + b, n_cols, True, *M.shift_rows(cos, sin, a + b))
    assert np.array_equal(two[:keep], one[:keep]) and np.array_equal(two[:keep], lane[:keep])
    hd = dh // 2
    d = two[keep:n_new].astype(np.float64) - one[keep:n_new].astype(np.float64)
    mag = np.hypot(lane[keep + a + b:, :hd], lane[keep + a + b:, hd:]).astype(np.float64)
    gap = float((np.hypot(d[:, :hd], d[:, hd:]) / np.maximum(mag, 1e-30)).max())
    print(f"two shifts against one: {gap:.3g} of the pair's magnitude")
    assert gap <= 4 * U * (a + b) + 3 * 2.001 * U
    # int8: the same places; every requantisation may cost a quantisation unit, so only the places are asserted
    q, sc = M.quantise(marks + f32(1))
    q2, sc2 = M.shift_i8(*M.shift_i8(q, sc, keep, a, n_cols, False), keep, b, n_cols - a, False)
    q1, sc1 = M.shift_i8(q, sc, keep, a + b, n_cols, False)
    assert np.array_equal(q2[:n_new], q1[:n_new]) and np.array_equal(sc2[:n_new], sc1[:n_new])


def test_the_wrappers_are_hip_only_and_check_their_arguments(oracle):
    """Session.shift / BatchSession.shift on an oracle session: a RuntimeError that says a HIP session is needed (like admit /
    fork), before anything else is looked at."""
    from zgml_amd import llama
    m = llama.Model(llama.preset("tiny"))
    s = llama.Session(m, oracle.backend_fns())
    with pytest.raises(RuntimeError, match="HIP session"):
        s.shift(4, 8, 32)
    bs = llama.BatchSession(m, oracle.backend_fns(), 2)
    with pytest.raises(RuntimeError, match="HIP session"):
        bs.shift(1, 4, 8, 32)
    bs.close(), s.close(), m.close()
