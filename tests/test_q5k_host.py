"""GGUF Q5_K without a GPU: the dequantiser on a closed-form block, the builder's Q5_K_M kinds against it, the forms the mirror takes."""
import ctypes as C

import numpy as np

from zgml_amd import Capabilities, DeviceOp, DeviceProgram, QuantizedWeightUpload, llama
from tests.q5k_cases import FORM_CASES, Q6K_WEIGHTS, model_config, q5k_blocks, q5k_parts
from tests.q6k_cases import q6k_weights


def test_dequantiser_on_a_block_in_closed_form():
    """qs[i] = i; qh = 0x35 (l < 16) / its complement: bit j is 1,0,1,0,1,1,0,0, which no shift or swap of j keeps; sixteen distinct
    sc and m that use the 6-bit unpack's top bits; d = 0.5, dmin = 0.25. A swapped j, a swapped nibble or a shifted high bit shows."""
    raw = q5k_blocks(np.random.default_rng(0), 1, 256, d=0.5, dmin=0.25)
    raw[0, 48:], raw[0, 16:32], raw[0, 32:48] = np.arange(128), 0x35, 0xCA
    raw[0, 4:8] = [(i + 1) | (i << 6) for i in range(4)]
    raw[0, 8:12] = [(10 + i) | ((3 - i) << 6) for i in range(4)]
    raw[0, 12:16] = [(5 + i) | ((3 + i) << 4) for i in range(4)]
    sc = [1, 2, 3, 4] + [5 + 17 * i for i in range(4)]
    m = [10, 11, 12, 13] + [3 + i + 16 * (3 - i) for i in range(4)]
    want = []
    for e in range(256):
        j, l = e >> 5, e & 31
        nibble = (l & 15) if j % 2 == 0 else 2 * (j >> 1) + (l >> 4)  # of byte 32 (j >> 1) + l
        high = ((0x35 >> j) & 1) ^ (l >> 4)
        want.append(0.5 * sc[j] * (nibble | high << 4) - 0.25 * m[j])
    a, b = q5k_parts(raw, 1, 256)
    assert np.array_equal((a - b)[0], np.array(want))
    assert QuantizedWeightUpload.from_gguf_blocks(raw, 1, 256, "q5_k").data.size == 176


def test_model_builder_emits_the_q5_k_m_mix_and_its_dense_twin():
    cfg = model_config()
    mq, md = llama.Model(cfg, llama.Q5_K_M_GGUF), llama.Model(cfg, llama.Q5_K_M_DENSE)
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == 15
    for i in range(15):
        qw = pq.qweights[i]
        six = i in Q6K_WEIGHTS
        assert qw.block_size == 256 and not qw.scales and qw.data_len == qw.rows * qw.cols // 256 * (210 if six else 176), i
        raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
        if six:
            ref = q6k_weights(raw, qw.rows, qw.cols)
            tol = 2.0 ** -24 * np.abs(ref)  # one f32 rounding
        else:
            a, b = q5k_parts(raw, qw.rows, qw.cols)
            ref, tol = a - b, 2.0 ** -23 * (np.abs(a) + np.abs(b))
            assert len(np.unique(raw.reshape(-1, 176)[:, 16:48])) == 256 and (a > 0).any() and (a < 0).any() and (b > 0).any() and (b < 0).any()
        up = pd.initial_uploads[i]  # the dense model's weight leaves come first, in weight order
        w = np.ctypeslib.as_array(C.cast(up.host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
        assert np.all(np.abs(w - ref) <= tol), i
    assert mq.quant_bytes()[0] == sum(pq.qweights[i].data_len for i in range(15))
    mq.close(), md.close()


def test_host_mirror_takes_exactly_the_documented_forms():
    for K, N, block, nbytes, want in FORM_CASES:
        qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, np.float32), K, N, block, gguf="q5_k")
        p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
        assert p.isSupportedBy(Capabilities.wgpu) is want, (K, N, block, nbytes)
