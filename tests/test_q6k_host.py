"""GGUF Q6_K without a GPU: the dequantiser on a closed-form block, the builder's Q4_K_M kinds against it, the forms the mirror takes."""
import ctypes as C

import numpy as np
import pytest

from zgml_amd import Capabilities, DeviceOp, DeviceProgram, QuantizedWeightUpload, llama
from tests.q4k_cases import q4k_parts
from tests.q6k_cases import FORM_CASES, Q6K_WEIGHTS, model_config, q6k_blocks, q6k_weights


def test_dequantiser_on_a_block_in_closed_form():
    """ql[i] = i, qh = 0xE4 (h = 0: high bits g) / 0x1B (h = 1: 3 - g), scales s - 8, d = 0.5: a swapped g, h or nibble shows"""
    raw = q6k_blocks(np.random.default_rng(0), 1, 256, d=0.5)
    raw[0, :128], raw[0, 128:160], raw[0, 160:192] = np.arange(128), 0xE4, 0x1B
    raw[0, 192:208] = (np.arange(16) - 8).astype(np.int8).view(np.uint8)
    want = []
    for e in range(256):
        h, g, l = e >> 7, (e >> 5) & 3, e & 31
        low = (l & 15) if g < 2 else 4 * h + 2 * (g & 1) + (l >> 4)  # nibbles of byte 64 h + 32 (g & 1) + l
        want.append(0.5 * (e // 16 - 8) * ((low | (g if h == 0 else 3 - g) << 4) - 32))
    assert np.array_equal(q6k_weights(raw, 1, 256)[0], np.array(want))


def test_model_builder_emits_the_q4_k_m_mix_and_its_dense_twin():
    cfg = model_config()
    mq, md = llama.Model(cfg, llama.Q4_K_M_GGUF), llama.Model(cfg, llama.Q4_K_M_DENSE)
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == 15
    for i in range(15):
        qw = pq.qweights[i]
        six = i in Q6K_WEIGHTS
        assert qw.block_size == 256 and not qw.scales and qw.data_len == qw.rows * qw.cols // 256 * (210 if six else 144), i
        raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
        if six:
            ref = q6k_weights(raw, qw.rows, qw.cols)
            sc = raw.reshape(-1, 210)[:, 192:208]
            assert len(np.unique(sc)) == 256 and (ref > 0).any() and (ref < 0).any()
            tol = 2.0 ** -24 * np.abs(ref)  # one f32 rounding
        else:
            a, b = q4k_parts(raw, qw.rows, qw.cols)
            ref, tol = a - b, 2.0 ** -23 * (np.abs(a) + np.abs(b))
        up = pd.initial_uploads[i]  # the dense model's weight leaves come first, in weight order
        w = np.ctypeslib.as_array(C.cast(up.host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
        assert np.all(np.abs(w - ref) <= tol), i
    assert mq.quant_bytes()[0] == sum(pq.qweights[i].data_len for i in range(15))
    mq.close(), md.close()


@pytest.mark.parametrize("K,N,block,nbytes,want", FORM_CASES)
def test_host_mirror_takes_exactly_the_documented_forms(K, N, block, nbytes, want):
    """scales absent, block_size 256, cols % 256 == 0: 144 B per 256 elements is Q4_K, 210 B Q6_K; nothing else over such bytes"""
    qw = QuantizedWeightUpload(np.zeros(nbytes, np.uint8), np.zeros(0, np.float32), K, N, block, gguf="q6_k")
    p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
    assert p.isSupportedBy(Capabilities.wgpu) is want
