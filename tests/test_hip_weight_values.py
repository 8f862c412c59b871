"""The quantized mat-vec / matmul kernels over the VALUE axis of their weights, through the route x class x profile matrix of
tests/weight_cases.py: negative, zero, -0.0, f16-subnormal and large block scales, the stored nibble 0 in every block, both ends of
int8 — what GGUF files hold and what no other test feeds a kernel (they all draw strictly positive, f16-normal scales).

Single-op DevicePrograms as run_both of tests/test_hip_qmatvec.py builds them: input at offset 4 with row stride K + 4, output at
offset 1 with row stride N + 5, -7 sentinels in front of, between and behind the rows, x = standard_normal. Shapes are the
smallest that take each route (zgml_amd/csrc: compile_program in runtime.hip, launch_qmatmul / launch_tile / launch_xdl2 /
launch_xdl4 / launch_xdl5 in qmatmul_tiles.hip; tests/test_weight_cases_host.py restates the conditions on the table):
  matvec-nol  M = 1, K < 2049 (ZGML_HIP_QMV_KON_MIN_K): the n-on-lanes body, all four packed classes; (32, 32) one unit, (100, 64)
              a K tail inside the last unit, (576, 192) several waves
  matvec-kon  M = 1, K >= 2049, Q4 values + f16 scales: compile_program packs K-on-lanes (QW_Q4K), qmatvec_kon_body's
              offset-binary form; (2080, 32), (2051, 32) odd K: scalar x loads and a padded last pair, (4096, 64)
  kon-rows    the same layout at M = 2 and 8 under OPT_SMALL_M_MATVEC = 8 (qmatvec_rows.hip; the plan text says so)
  tile        M > 1 and not xdl2_applies (f32 scales or Q8 values): qmatmul_tile_kernel<ST, Q4, 1 | 2> at M = 2 / 17
  xdl2        M = 2, 17, 32 over Q4 + f16: split_a + qmatmul_xdl2_kernel<1 | 2> (1 workgroup-column < 40: not xdl5; K too short
              for the two-m-tile K split)
  xdl5        576 x 10240: cdiv(320 block-columns, 8) = 40 workgroup-columns, the shared-A form at M = 5 (RT 1) and 32 (RT 2)
  xdl4        M = 33 (RT 4), 65 (RT 8); K = 576: 5 steps, one K slice; K = 4096: 32 steps cut into 4 slices with ordered fan-in
  xdl4-m32    M = 32 on the K-split kernel at two m-tiles needs sk >= 2 slices of >= 16 steps: (4096, 512) gives 4 slices of 8
              steps and stays with xdl2, so the case is (8192, 512): 64 steps, 4 slices of 16 (256 CUs / 16 block-columns)
  grouped     three weights over the same rows: one launch (M = 1: qmv parts 3; M = 5: launch_qmatmul_group -> xdl2 with parts)
  raw         N = 48 or block size 4: qmatmul_raw_kernel, same loop order as the reference, so also bit-equal to the oracle
  gguf-pack   raw Q4_0 / Q8_0 file blocks through pack_gguf_kernel (n-on-lanes at (576, 192), K-on-lanes at (2080, 32))

Per case and profile, every output row and column:
  1. |got - want64| <= 2e-5 * bound64 + 1e-30 against the float64 reference (the project's tolerance);
  2. got == 0 exactly where bound64 == 0 (zero scales, all-zero data);
  3. sentinels untouched, everything finite;
  4. xdl4 / xdl5 (ordered fan-in): a second execution repeats the bits;
  5. gguf_* classes: bit-equal to the expanded upload (int8 + f32 scales) of the same blocks;
  6. sign symmetry. The VALU forms (every M = 1 mat-vec, kon-rows, raw): `negated` == -`positive` element by element (0 == -0
     accepted) — f32 multiply / add / fma, the fp8 and SDWA converts and the f16 conversion of the packers all round
     sign-symmetrically. The matrix-core forms (tile, xdl2, xdl4, xdl5 and the M > 1 grouped / gguf-pack cases) are legitimately
     NOT symmetric: v_mfma_f32_16x16x32_bf16 adds its 32 exact products to the accumulator with a rounding that is not an odd
     function — measured: negating the scales, negating x, or (Q8) negating the data each give the SAME bits as one another and
     differ from the negated `positive` result in the last bits (up to 2e-5 relative on cancelling sums), in the A-side-scale
     form and the B-side-scale forms alike, and repeatably. For those the check is the sharper half that survives: `negated`
     weights over x == `positive` weights over -x BIT FOR BIT — both feed the matrix cores the same products, so every sign
     carried through a scale (classify / pack / xdl_prep_b's truncating split / the A-side multiply) must arrive exactly as a
     sign carried through x does. Checks 1 - 5 hold for every form."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload, capi
from tests import weight_cases as WC

pytestmark = pytest.mark.gpu
f32 = np.float32
IN_OFF, DST_OFF = 4, 1
_positive_results = {}


def layout(c, N):
    in_rs = c.K + 4 if c.M > 1 else 0
    dst_rs = N + 5 if c.M > 1 else 0
    return in_rs, dst_rs, DST_OFF + (c.M - 1) * (dst_rs or N) + N + 2


def program(c, uploads, x):
    in_rs = layout(c, c.N)[0]
    xin = np.full(IN_OFF + (c.M - 1) * (in_rs or c.K) + c.K + 3, 99, f32)
    for m in range(c.M):
        xin[IN_OFF + m * (in_rs or c.K):][:c.K] = x.reshape(c.M, c.K)[m]
    sizes, ups, ops = [xin.size], [ProgramIO(0, xin)], []
    for t, N in enumerate(c.Ns):
        _, dst_rs, dst_len = layout(c, N)
        sizes.append(dst_len)
        ups.append(ProgramIO(1 + t, np.full(dst_len, WC.SENTINEL, f32)))
        ops.append(DeviceOp.qmatmul(1 + t, 0, t, c.M, N, c.K, IN_OFF, in_rs, DST_OFF, dst_rs))
    return DeviceProgram(ops=ops, buffer_sizes=sizes, initial_uploads=ups, qweights=uploads)


def execute(be, c, prog, times=1):
    """[[buffer per part] per execution], and the plan text"""
    if c.small_m:
        be.set_option(capi.OPT_SMALL_M_MATVEC, 8)
    try:
        h = be.compileProgram(prog)
    finally:
        if c.small_m:
            be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    assert h, be.last_error()
    try:
        text = be.planText(h)
        runs = []
        for _ in range(times):
            outs = [ProgramIO(1 + t, np.zeros(prog.buffer_sizes[1 + t], f32)) for t in range(len(c.Ns))]
            be.executeProgram(h, [], outs)
            assert not be.last_error(), be.last_error()
            runs.append([io.host for io in outs])
    finally:
        be.freeProgram(h)
    return runs, text


def rows_of(c, N, buf):
    dst_rs = layout(c, N)[1]
    return np.stack([buf[DST_OFF + m * (dst_rs or N):][:N] for m in range(c.M)])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_case(be, oracle, c, profile, phase, x_sign=1.0):
    """checks 1 - 5 for one weight set; ([rows per part], worst |delta| / bound64)"""
    what = f"{c.id} {profile} phase {phase}" + (" over -x" if x_sign < 0 else "")
    weights = WC.case_weights(c, profile, phase)
    x = WC.case_x(c) * f32(x_sign)
    expanded = [QuantizedWeightUpload(np.array(d), np.array(s), c.K, N, c.bs) for (d, s), N in zip(weights, c.Ns)]
    gguf = c.cls.startswith("gguf_")
    uploads = [QuantizedWeightUpload.from_gguf_blocks(WC.gguf_blocks(c.cls, d, s), c.K, N, c.cls[5:]) for (d, s), N in zip(weights, c.Ns)] if gguf else expanded
    prog = program(c, uploads, x)
    assert be.supportsProgram(prog), what
    runs, text = execute(be, c, prog, times=2 if c.ordered else 1)
    lines = text.strip().splitlines()
    if c.route == "kon-rows":
        assert "qmatvec-kon-rows" in text, text
    if c.route == "grouped":
        assert len(lines) == 1 and f"ops {len(c.Ns)} " in lines[0], text
    worst, rows = 0.0, []
    for t, N in enumerate(c.Ns):
        buf = runs[0][t]
        got = rows_of(c, N, buf)
        want, bound = WC.reference(*weights[t], x, c.M, N, c.K, c.bs)
        assert np.all(np.isfinite(buf)), what
        mask = np.ones(buf.size, bool)  # 3. everything outside the rows still holds the sentinel
        dst_rs = layout(c, N)[1]
        for m in range(c.M):
            mask[DST_OFF + m * (dst_rs or N):][:N] = False
        assert np.all(buf[mask] == WC.SENTINEL), what
        err = np.abs(got.astype(np.float64) - want)
        live = bound > 0
        ratio = float(np.max(err[live] / bound[live], initial=0.0))
        worst = max(worst, ratio)
        assert np.all(err <= WC.TOL * bound + WC.FLOOR), (what, t, ratio)  # 1.
        assert np.all(got[~live] == 0), (what, t)  # 2.
        if c.ordered:
            assert same_bits(buf, runs[1][t]), (what, t)  # 4.
        rows.append(got)
    if gguf:  # 5.
        again, _ = execute(be, c, program(c, expanded, x))
        for t in range(len(c.Ns)):
            assert same_bits(runs[0][t], again[0][t]), (what, t)
    if c.route == "raw":  # the k-sequential kernel repeats the reference's loop order
        for t, N in enumerate(c.Ns):
            assert np.array_equal(runs[0][t], oracle.run_program(prog, 1 + t, prog.buffer_sizes[1 + t])), (what, t)
    return rows, worst


@pytest.mark.parametrize("profile", WC.PROFILES)
@pytest.mark.parametrize("case_id", WC.CASE_IDS)
def test_weight_values(hip_backend, oracle, case_id, profile):
    c = WC.CASES[WC.CASE_IDS.index(case_id)]
    worst, sym = 0.0, "-"
    for phase in WC.variants(profile, c.N, c.bs):
        rows, w = run_case(hip_backend, oracle, c, profile, phase)
        worst = max(worst, w)
    if profile == "positive":
        _positive_results[case_id] = rows
    if profile == "negated" and not c.mfma:  # 6., VALU forms
        pos = _positive_results.get(case_id) or run_case(hip_backend, oracle, c, "positive", 0)[0]
        for t, (p, n) in enumerate(zip(pos, rows)):
            bad = np.flatnonzero((n != -p).ravel())
            assert bad.size == 0, f"{case_id}: part {t}: negated scales do not give the negated result at {bad.size} elements, first {bad[:8]}: {n.ravel()[bad[:4]]} vs {-p.ravel()[bad[:4]]}"
        sym = "bit-for-bit"
    if profile == "negated" and c.mfma:  # 6., matrix-core forms
        flipped = run_case(hip_backend, oracle, c, "positive", 0, x_sign=-1.0)[0]
        for t, (p, n) in enumerate(zip(flipped, rows)):
            bad = np.flatnonzero((n.view(np.uint32) != p.view(np.uint32)).ravel())
            assert bad.size == 0, f"{case_id}: part {t}: negated scales and negated x differ at {bad.size} elements, first {bad[:8]}: {n.ravel()[bad[:4]]} vs {p.ravel()[bad[:4]]}"
        pos = _positive_results.get(case_id)
        sym = "equals-negated-x-bit-for-bit" + ("" if pos is None else f" (vs -positive: {sum(int(np.sum(n != -p)) for p, n in zip(pos, rows))} of {sum(n.size for n in rows)} elements differ)")
    print(f"\nWV route={c.route} case={case_id} profile={profile} worst={worst:.3e} sym={sym}")
