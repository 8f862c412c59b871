"""GGUF IQ4_XS weights on the MI355X (zgml_amd/csrc/sb_kernels.hip, format Sb4x): mat-vecs and matmuls against float64 over the super-block
family's shapes and the format's pins, the upload forms the device takes, a program that mixes it with Q6_K and Q4_K, and the IQ4_XS
model against the oracle on its dense twin. Per output |y - x a| <= 2e-5 * sum_k |x[k]| |a| + 1e-30: sb_cases.check."""
import numpy as np
import pytest

from zgml_amd import DeviceOp, DeviceProgram, ProgramIO, QuantizedWeightUpload, llama
from tests.iq4xs_cases import PINS, iq4xs_blocks, iq4xs_parts
from tests.sb_cases import F16_MAX, SHAPES, blocks, check, form_program, model_config, parts, qmatmul, run
from tests.test_iq4xs_host import FORM_CASES

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize("M,K,N,strided,pin", [(*s, None) for s in SHAPES] + [(M, 96, 256, False, pin) for M in (1, 5) for pin in PINS])
def test_matmul_against_float64(hip_backend, M, K, N, strided, pin):
    rng = np.random.default_rng(M * 1000003 + K * 131 + N)
    raw = iq4xs_blocks(rng, K, N, **PINS.get(pin, {}))
    a, b = iq4xs_parts(raw, K, N)
    x = rng.standard_normal((M, K)).astype(f32)
    got = qmatmul(hip_backend, QuantizedWeightUpload.from_gguf_blocks(raw, K, N, "iq4_xs"), x, M, K, N, strided)
    if pin == "max":
        assert a.min() == a.max() == 4064 * F16_MAX
    elif pin == "zero":
        assert not a.any() and not got.any()
    elif pin == "table ends":  # every item: columns 0..15 take -127, columns 16..31 take 113
        i = a.reshape(K, N // 32, 32)
        assert a.any() and np.array_equal(i[:, :, :16] * 113, i[:, :, 16:] * -127) and (i[:, :, :1] == i[:, :, :16]).all()
    assert np.isfinite(got).all()
    check(got, x, a, b)


def test_forms_the_device_takes(hip_backend):
    for K, N, block, nbytes, want in FORM_CASES:
        assert hip_backend._lib.zgml_hip_program_supported(form_program("iq4_xs", K, N, block, nbytes).to_c()[0]) == int(want), (K, N, block, nbytes)


def test_mixed_program_and_run_to_run_identity(hip_backend):
    """IQ4_XS beside Q6_K and Q4_K in one program and one execute, at a K-split shape each; a second execute: the same bytes"""
    rng = np.random.default_rng(11)
    kinds, Ks, N = ["iq4_xs", "q6_k", "q4_k"], [577, 577, 261], 256
    raws = [iq4xs_blocks(rng, Ks[0], N)] + [blocks(kind, rng, K, N) for kind, K in zip(kinds[1:], Ks[1:])]
    refs = [iq4xs_parts(raws[0], Ks[0], N)] + [parts(kind, raw, K, N) for kind, raw, K in zip(kinds[1:], raws[1:], Ks[1:])]
    xs = [rng.standard_normal(K).astype(f32) for K in Ks]
    prog = DeviceProgram(ops=[DeviceOp.qmatmul(3 + i, i, i, 1, N, K) for i, K in enumerate(Ks)], buffer_sizes=Ks + [N] * 3,
                         initial_uploads=[ProgramIO(i, x) for i, x in enumerate(xs)],
                         qweights=[QuantizedWeightUpload.from_gguf_blocks(raw, K, N, kind) for raw, K, kind in zip(raws, Ks, kinds)])
    first, second = run(hip_backend, prog, [[(3 + i, N) for i in range(3)]] * 2)
    for y, y2, x, (a, b) in zip(first, second, xs, refs):
        check(y[None, :], x[None, :], a, b)
        assert np.array_equal(y, y2)


@pytest.mark.parametrize("T", [1, 8])
def test_model_matches_the_dense_oracle(hip_backend, oracle, T):
    """T = 1: six decode steps; T = 8: two prefill chunks; tokens equal, logits within 2e-4 of the logit range"""
    cfg = model_config()
    m_hip, m_ref = llama.Model(cfg, llama.IQ4_XS_GGUF, token_len=T), llama.Model(cfg, llama.IQ4_XS_DENSE, token_len=T)
    qws = [m_hip.program.qweights[i] for i in range(m_hip.program.n_qweights)]
    assert [q.data_len * 256 // (q.rows * q.cols) for q in qws] == [136] * 14 + [210]
    s_hip, s_ref = llama.Session(m_hip, llama.hip_backend_fns(hip_backend)), llama.Session(m_ref, oracle.backend_fns())
    tok = 3
    for it in range(6 if T == 1 else 2):
        toks = [(7 * i + 3 + it) % cfg.vocab_size for i in range(T)]
        (t_hip, l_hip), (t_ref, l_ref) = [s.step(tok, it) if T == 1 else s.prefill(toks, it * T) for s in (s_hip, s_ref)]
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert t_hip == t_ref and np.abs(l_hip - l_ref).max() / np.abs(l_ref).max() < 2e-4, (it, t_hip, t_ref)
        tok = t_ref
    s_hip.close(), s_ref.close(), m_hip.close(), m_ref.close()


def test_resident_decode_equals_stepping(hip_backend):
    m = llama.Model(model_config(), llama.IQ4_XS_GGUF)
    s = llama.Session(m, llama.hip_backend_fns(hip_backend))
    s.resident_setup(hip_backend)
    got, (want, _) = s.resident_decode(5, 0, 16), s.decode(5, 0, 16)
    assert not hip_backend.last_error(), hip_backend.last_error()
    assert got.tolist() == want.tolist()
    s.close(), m.close()
