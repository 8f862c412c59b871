"""GGUF IQ4_XS without a GPU: tests/iq4xs_cases.py's dequantiser on a closed-form block (what pins the bit order), the host model
builder's IQ4_XS mix (zgml_amd/csrc/iq4xs.h on the CPU) against it, the upload forms the host mirror takes."""
import ctypes as C

import numpy as np

from zgml_amd import Capabilities, QuantizedWeightUpload, llama
from tests.iq4xs_cases import KVALUES, iq4xs_blocks, iq4xs_parts
from tests.sb_cases import form_program, model_config

LS = [(13 * ib + 5) & 15 | ((ib + (ib >> 2)) & 3) << 4 for ib in range(8)]  # eight distinct 6-bit scales over every value of the top two bits
QS = [(i * 0x1D + (i >> 4)) & 255 for i in range(128)]  # the two nibbles of a byte differ, and from byte to byte
# (K, N, block_size, data_len, accepted): the exact byte count; a byte too many; cols = 384; blocks of 32 (8704 is neither 512 * 18 nor 512 * 34)
FORM_CASES = [(64, 256, 256, 64 * 136, True), (64, 256, 256, 64 * 136 + 1, False), (64, 384, 256, 96 * 136, False), (64, 256, 32, 64 * 136, False)]


def test_dequantiser_on_a_block_in_closed_form():
    """d = 0.5 over bytes set by hand, against the element-by-element statement of the format"""
    raw = iq4xs_blocks(np.random.default_rng(0), 1, 256, d=0.5, scales_h=sum((LS[ib] >> 4) << 2 * ib for ib in range(8)),
                       scales_l=[LS[2 * i] & 15 | (LS[2 * i + 1] & 15) << 4 for i in range(4)], qs=QS)
    assert len(set(LS)) == 8 and {ls >> 4 for ls in LS} == {0, 1, 2, 3}
    want = [0.5 * (LS[e >> 5] - 32) * KVALUES[(QS[16 * (e >> 5) + (e & 15)] >> 4 * ((e >> 4) & 1)) & 15] for e in range(256)]
    assert np.array_equal(iq4xs_parts(raw, 1, 256)[0][0], np.array(want))
    assert QuantizedWeightUpload.from_gguf_blocks(raw, 1, 256, "iq4_xs").data.size == 136


def test_model_builder_emits_the_mix_and_its_dense_twin():
    """kind 14 over the all-256 model (4 heads, 4 kv heads, L/8 = 0): IQ4_XS everywhere under the Q6_K head; the dense kind: the same values
    in f32 (one rounding: the format has no min term); d of both signs"""
    mq, md = llama.Model(model_config(), llama.IQ4_XS_GGUF), llama.Model(model_config(), llama.DENSE_TWIN[llama.IQ4_XS_GGUF])
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == 15
    for i, nbytes in enumerate([136] * 14 + [210]):
        qw = pq.qweights[i]
        assert qw.block_size == 256 and not qw.scales and qw.scales_len == 0 and qw.data_len == qw.rows * qw.cols // 256 * nbytes, i
        if nbytes == 136:
            raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
            a, _ = iq4xs_parts(raw, qw.rows, qw.cols)
            assert len(np.unique(raw.reshape(-1, 136)[:, 1] >> 7)) == 2, i
            w = np.ctypeslib.as_array(C.cast(pd.initial_uploads[i].host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
            assert a.any() and np.all(np.abs(w - a) <= 2.0 ** -24 * np.abs(a)), i
    mq.close(), md.close()


def test_host_mirror_takes_exactly_the_documented_forms():
    for K, N, block, nbytes, want in FORM_CASES:
        assert form_program("iq4_xs", K, N, block, nbytes).isSupportedBy(Capabilities.wgpu) is want, (K, N, block, nbytes)
