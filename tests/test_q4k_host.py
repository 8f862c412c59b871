"""GGUF Q4_K without a GPU: tests/q4k_cases.py against a hand-computed super-block, the host model builder's Q4_K kinds
(zgml_amd/csrc/q4k.h on the CPU) against that dequantiser, and the upload forms the host mirror takes."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import Capabilities, DeviceOp, DeviceProgram, QuantizedWeightUpload, llama
from tests.q4k_cases import q4k_blocks, q4k_parts

GOLDEN = json.loads((Path(__file__).parent / "golden" / "q4k_block.json").read_text())


def test_dequantiser_and_generator_agree_with_a_hand_computed_block():
    blk = np.array(GOLDEN["block"], np.uint8)
    a, b = q4k_parts(blk, 1, 256)
    assert np.array_equal((a - b)[0], np.array(GOLDEN["values"]))
    d, dmin = (float(v) for v in blk[0:4].view(np.float16))
    gen = q4k_blocks(np.random.default_rng(0), 2, 256, d=d, dmin=dmin, scale_byte=0xFF, q_byte=0x21)  # sc = m = 63; nibbles 1 | 2
    assert gen.shape == (2, 144) and np.array_equal(gen[1, :4], blk[:4])
    a, b = q4k_parts(gen, 2, 256)
    assert np.array_equal((a - b)[1], np.tile(np.repeat([1.0, 2.0], 32), 4) * 63 * d - 63 * dmin)


def test_model_builder_emits_super_blocks_and_their_dense_twin():
    """Q4_K_GGUF: super-blocks where N % 256 == 0, Q4_0 blocks elsewhere; Q4_K_DENSE: the same values in f32 (two roundings)"""
    cfg = llama.preset("tiny")  # d_model 128 (kv width 64): Q4_0 blocks; d_ff 256: gate / up are Q4_K
    mq, md = llama.Model(cfg, llama.Q4_K_GGUF), llama.Model(cfg, llama.Q4_K_DENSE)
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == 14
    for i in range(14):
        qw = pq.qweights[i]
        sb = qw.cols % 256 == 0
        assert qw.block_size == (256 if sb else 32) and not qw.scales and qw.scales_len == 0
        assert qw.data_len == qw.rows * qw.cols // 256 * 144  # (= rows * cols / 32 * 18)
        if not sb:
            continue
        raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
        a, b = q4k_parts(raw, qw.rows, qw.cols)
        up = pd.initial_uploads[i]  # the dense model's weight leaves come first, in weight order
        w = np.ctypeslib.as_array(C.cast(up.host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
        assert np.all(np.abs(w - (a - b)) <= 2.0 ** -23 * (np.abs(a) + np.abs(b)))
        sc = raw.reshape(-1, 144)[:, 4:16]
        assert len(np.unique(sc & 63)) == 64 and (a > 0).any() and (a < 0).any() and (b > 0).any() and (b < 0).any()
    assert mq.quant_bytes()[0] == sum(pq.qweights[i].data_len for i in range(14))
    mq.close(), md.close()


@pytest.mark.parametrize("K,N,block,extra,want", [(64, 256, 256, 0, True), (64, 256, 32, 0, True), (64, 384, 256, 0, False),
                                                  (64, 256, 256, 1, False), (64, 256, 64, 0, False)])
def test_host_mirror_takes_exactly_the_documented_forms(K, N, block, extra, want):
    """scales absent: block_size 256 with cols % 256 == 0 and 144 B per 256 elements is Q4_K, 32 over the same bytes Q4_0"""
    qw = QuantizedWeightUpload(np.zeros(K * N // 256 * 144 + extra, np.uint8), np.zeros(0, np.float32), K, N, block,
                               gguf="q4_k" if block == 256 else "q4_0")
    p = DeviceProgram(ops=[DeviceOp.qmatmul(1, 0, 0, 1, N, K)], buffer_sizes=[K, N], qweights=[qw])
    assert p.isSupportedBy(Capabilities.wgpu) is want
