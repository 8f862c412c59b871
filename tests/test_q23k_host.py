"""GGUF Q3_K / Q2_K without a GPU: the dequantisers on closed-form blocks (what pins the bit order), the builder's mixes, the mirror's forms."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import Capabilities, DeviceOp, DeviceProgram, QuantizedWeightUpload, llama
from tests.q23k_cases import BYTES, FORM_CASES, blocks, parts
from tests.q4k_cases import q4k_parts
from tests.q5k_cases import q5k_parts
from tests.q6k_cases import model_config, q6k_weights

QS = [(i * 0x1B + (i >> 3)) & 255 for i in range(64)]  # the four 2-bit fields of a byte differ, and from byte to byte


@pytest.mark.parametrize("fmt", list(BYTES))
def test_dequantiser_on_a_block_in_closed_form(fmt):
    # hmask = 0x35 (l < 16) / its complement: bit g is 1,0,1,0,1,1,0,0, which no shift or swap of g keeps; sixteen distinct 6-bit scales
    # over every value of the top two bits (Q2_K: sixteen distinct nibble pairs); d = 0.5, dmin = 0.25
    sc6 = [(5 * s + 3) & 15 | ((s + (s >> 2)) & 3) << 4 for s in range(16)]
    pairs = [((7 * s + 3) & 15, (11 * s + 5) & 15) for s in range(16)]
    raw = blocks(fmt, np.random.default_rng(0), 1, 256, d=0.5, dmin=0.25)
    if fmt == "q3_k":
        raw[0, :16], raw[0, 16:32], raw[0, 32:96] = 0x35, 0xCA, QS
        raw[0, 96:104] = [sc6[i] & 15 | (sc6[i + 8] & 15) << 4 for i in range(8)]
        raw[0, 104:108] = [sum((sc6[4 * g + j] >> 4) << 2 * g for g in range(4)) for j in range(4)]
    else:
        raw[0, :16], raw[0, 16:80] = [sc | m << 4 for sc, m in pairs], QS
    want = []
    for e in range(256):
        low = (QS[32 * (e >> 7) + (e & 31)] >> 2 * ((e >> 5) & 3)) & 3
        high = ((0x35 >> (e >> 5)) & 1) ^ ((e & 31) >> 4)
        want.append(0.5 * (sc6[e >> 4] - 32) * (low + 4 * high - 4) if fmt == "q3_k" else 0.5 * pairs[e >> 4][0] * low - 0.25 * pairs[e >> 4][1])
    a, b = parts(fmt, raw, 1, 256)
    assert np.array_equal((a - b)[0], np.array(want))
    assert QuantizedWeightUpload.from_gguf_blocks(raw, 1, 256, fmt).data.size == BYTES[fmt]


# the bytes per weight (per layer q, k, v, o, gate, up, down; then the head) of the two-layer model (L/16 = L/8 = 0) per kind
MIXES = {llama.Q3_K_M_GGUF: [110, 110, 176, 144, 110, 110, 144] * 2 + [210], llama.Q2_K_GGUF: [84, 84, 110, 110, 84, 84, 110] * 2 + [210]}
PARTS = {84: lambda *a: parts("q2_k", *a), 110: lambda *a: (parts("q3_k", *a)[0], 0.0), 144: q4k_parts, 176: q5k_parts, 210: lambda *a: (q6k_weights(*a), 0.0)}


@pytest.mark.parametrize("kind", list(MIXES))
def test_model_builder_emits_the_mix_and_its_dense_twin(kind):
    mq, md = llama.Model(model_config(), kind), llama.Model(model_config(), kind + 1)  # (kinds 10 / 12; the dense twins are 11 / 13)
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == 15
    for i, nbytes in enumerate(MIXES[kind]):
        qw = pq.qweights[i]
        assert qw.block_size == 256 and not qw.scales and qw.data_len == qw.rows * qw.cols // 256 * nbytes, i
        raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
        a, b = PARTS[nbytes](raw, qw.rows, qw.cols)
        assert (a > 0).any() and (a < 0).any() and len(np.unique(raw.reshape(-1, nbytes)[:, 16:32])) == 256  # d of both signs, hashed bytes
        up = pd.initial_uploads[i]  # the dense model's weight leaves come first, in weight order
        w = np.ctypeslib.as_array(C.cast(up.host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
        tol = 2.0 ** -23 * (np.abs(a) + np.abs(b)) if np.ndim(b) else 2.0 ** -24 * np.abs(a)  # two f32 roundings, or (no min term) one
        assert np.all(np.abs(w - (a - b)) <= tol), i
    assert mq.quant_bytes()[0] == sum(pq.qweights[i].data_len for i in range(15))
    mq.close(), md.close()


@pytest.mark.parametrize("fmt", list(BYTES))
def test_host_mirror_takes_exactly_the_documented_forms(fmt):
    for K, N, block, nbytes, want in FORM_CASES[fmt]:
        qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, np.float32), K, N, block, gguf=fmt)
        p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
        assert p.isSupportedBy(Capabilities.wgpu) is want, (K, N, block, nbytes)
