"""The GGUF super-block formats without a GPU: tests/sb_cases.py's dequantisers on closed-form blocks (what pins the bit order), the
host model builder's mixes (zgml_amd/csrc/q2k.h .. q6k.h on the CPU) against those dequantisers, the upload forms the host mirror takes."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import Capabilities, QuantizedWeightUpload, llama
from tests.sb_cases import BY_BYTES, FORM_CASES, FORMATS, MIXES, blocks, form_program, model_config, parts

GOLDEN = json.loads((Path(__file__).parent / "golden" / "q4k_block.json").read_text())
QS = [(i * 0x1B + (i >> 3)) & 255 for i in range(64)]  # the four 2-bit fields of a byte differ, and from byte to byte
# sixteen distinct 6-bit scales over every value of the top two bits (Q3_K); sixteen distinct nibble pairs (Q2_K)
SC6 = [(5 * s + 3) & 15 | ((s + (s >> 2)) & 3) << 4 for s in range(16)]
PAIRS = [((7 * s + 3) & 15, (11 * s + 5) & 15) for s in range(16)]


def test_q4k_dequantiser_and_generator_agree_with_a_hand_computed_block():
    blk = np.array(GOLDEN["block"], np.uint8)
    a, b = parts("q4_k", blk, 1, 256)
    assert np.array_equal((a - b)[0], np.array(GOLDEN["values"]))
    d, dmin = (float(v) for v in blk[0:4].view(np.float16))
    gen = blocks("q4_k", np.random.default_rng(0), 2, 256, d=d, dmin=dmin, scales=0xFF, qs=0x21)  # sc = m = 63; nibbles 1 | 2
    assert gen.shape == (2, 144) and np.array_equal(gen[1, :4], blk[:4])
    a, b = parts("q4_k", gen, 2, 256)
    assert np.array_equal((a - b)[1], np.tile(np.repeat([1.0, 2.0], 32), 4) * 63 * d - 63 * dmin)


def closed_q5k(raw):
    """qs[i] = i; qh = 0x35 (l < 16) / its complement: bit j is 1,0,1,0,1,1,0,0, which no shift or swap of j keeps; sixteen distinct
    sc and m that use the 6-bit unpack's top bits. A swapped j, a swapped nibble or a shifted high bit shows."""
    raw[0, 48:], raw[0, 16:32], raw[0, 32:48] = np.arange(128), 0x35, 0xCA
    raw[0, 4:8] = [(i + 1) | (i << 6) for i in range(4)]
    raw[0, 8:12] = [(10 + i) | ((3 - i) << 6) for i in range(4)]
    raw[0, 12:16] = [(5 + i) | ((3 + i) << 4) for i in range(4)]
    sc = [1, 2, 3, 4] + [5 + 17 * i for i in range(4)]
    m = [10, 11, 12, 13] + [3 + i + 16 * (3 - i) for i in range(4)]
    for e in range(256):
        j, l = e >> 5, e & 31
        nibble = (l & 15) if j % 2 == 0 else 2 * (j >> 1) + (l >> 4)  # of byte 32 (j >> 1) + l
        high = ((0x35 >> j) & 1) ^ (l >> 4)
        yield 0.5 * sc[j] * (nibble | high << 4) - 0.25 * m[j]


def closed_q6k(raw):
    """ql[i] = i, qh = 0xE4 (h = 0: high bits g) / 0x1B (h = 1: 3 - g), scales s - 8: a swapped g, h or nibble shows"""
    raw[0, :128], raw[0, 128:160], raw[0, 160:192] = np.arange(128), 0xE4, 0x1B
    raw[0, 192:208] = (np.arange(16) - 8).astype(np.int8).view(np.uint8)
    for e in range(256):
        h, g, l = e >> 7, (e >> 5) & 3, e & 31
        low = (l & 15) if g < 2 else 4 * h + 2 * (g & 1) + (l >> 4)  # nibbles of byte 64 h + 32 (g & 1) + l
        yield 0.5 * (e // 16 - 8) * ((low | (g if h == 0 else 3 - g) << 4) - 32)


def closed_q3k(raw):
    """hmask = 0x35 (l < 16) / its complement: bit g is 1,0,1,0,1,1,0,0, which no shift or swap of g keeps; the scales SC6"""
    raw[0, :16], raw[0, 16:32], raw[0, 32:96] = 0x35, 0xCA, QS
    raw[0, 96:104] = [SC6[i] & 15 | (SC6[i + 8] & 15) << 4 for i in range(8)]
    raw[0, 104:108] = [sum((SC6[4 * g + j] >> 4) << 2 * g for g in range(4)) for j in range(4)]
    for e in range(256):
        low = (QS[32 * (e >> 7) + (e & 31)] >> 2 * ((e >> 5) & 3)) & 3
        high = ((0x35 >> (e >> 5)) & 1) ^ ((e & 31) >> 4)
        yield 0.5 * (SC6[e >> 4] - 32) * (low + 4 * high - 4)


def closed_q2k(raw):
    raw[0, :16], raw[0, 16:80] = [sc | m << 4 for sc, m in PAIRS], QS
    for e in range(256):
        low = (QS[32 * (e >> 7) + (e & 31)] >> 2 * ((e >> 5) & 3)) & 3
        yield 0.5 * PAIRS[e >> 4][0] * low - 0.25 * PAIRS[e >> 4][1]


CLOSED = {"q5_k": closed_q5k, "q6_k": closed_q6k, "q3_k": closed_q3k, "q2_k": closed_q2k}  # (Q4_K: the golden block above)


@pytest.mark.parametrize("fmt", list(CLOSED))
def test_dequantiser_on_a_block_in_closed_form(fmt):
    """d = 0.5 (dmin = 0.25) over bytes set by hand, against the element-by-element statement of the format"""
    raw = blocks(fmt, np.random.default_rng(0), 1, 256, **{h: v for h, v in (("d", 0.5), ("dmin", 0.25)) if h in FORMATS[fmt].halves})
    want = list(CLOSED[fmt](raw))
    a, b = parts(fmt, raw, 1, 256)
    assert np.array_equal((a - b)[0], np.array(want))
    assert QuantizedWeightUpload.from_gguf_blocks(raw, 1, 256, fmt).data.size == FORMATS[fmt].nbytes


@pytest.mark.parametrize("kind,cfg", [(kind, "all-256") for kind in MIXES] + [(llama.Q4_K_GGUF, "tiny")])
def test_model_builder_emits_the_mix_and_its_dense_twin(kind, cfg):
    """the gguf kind: super-blocks of the mix's type where N % 256 == 0, Q4_0 file blocks elsewhere (preset "tiny": d_model 128, kv width
    64; d_ff 256: gate / up are Q4_K); the dense kind: the same values in f32 (two roundings; without a min term one)"""
    cfg, want = (model_config(), MIXES[kind]) if cfg == "all-256" else (llama.preset("tiny"), [144] * 14)
    mq, md = llama.Model(cfg, kind), llama.Model(cfg, llama.DENSE_TWIN[kind])
    pq, pd = mq.program, md.program
    assert pq.n_ops == pd.n_ops and pd.n_qweights == 0 and pq.n_qweights == len(want)
    for i, nbytes in enumerate(want):
        qw = pq.qweights[i]
        sb = qw.cols % 256 == 0
        assert qw.block_size == (256 if sb else 32) and not qw.scales and qw.scales_len == 0, i
        assert qw.data_len == qw.rows * qw.cols // 256 * nbytes, i  # (Q4_0: 144 B per 256 = 18 B per 32)
        if not sb:
            continue
        fmt = BY_BYTES[nbytes]
        raw = np.ctypeslib.as_array(C.cast(qw.data, C.POINTER(C.c_uint8)), shape=(qw.data_len,))
        a, b = fmt.parts(raw, qw.rows, qw.cols)
        assert (a > 0).any() and (a < 0).any() and (not fmt.has_min or ((b > 0).any() and (b < 0).any())), i  # d (dmin) of both signs
        for lo, hi, mask in fmt.hashed:  # hashed bytes: every value shows once they outnumber the values 16 to 1 (a miss: (mask + 1) e^-16 < 3e-5)
            seen = raw.reshape(-1, nbytes)[:, lo:hi] & mask
            assert seen.size < 16 * (mask + 1) or len(np.unique(seen)) == mask + 1, (i, lo, hi)
        up = pd.initial_uploads[i]  # the dense model's weight leaves come first, in weight order
        w = np.ctypeslib.as_array(C.cast(up.host_ptr, C.POINTER(C.c_float)), shape=(qw.rows, qw.cols))
        tol = 2.0 ** -23 * (np.abs(a) + np.abs(b)) if fmt.has_min else 2.0 ** -24 * np.abs(a)
        assert np.all(np.abs(w - (a - b)) <= tol), i
    assert mq.quant_bytes()[0] == sum(pq.qweights[i].data_len for i in range(len(want)))
    mq.close(), md.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_host_mirror_takes_exactly_the_documented_forms(fmt):
    """scales absent, block_size 256, cols % 256 == 0 and the bytes of one of the five types per 256 elements: that type; Q4_K's bytes
    under block_size 32: Q4_0; nothing else"""
    for K, N, block, nbytes, want in FORM_CASES[fmt]:
        assert form_program(fmt, K, N, block, nbytes).isSupportedBy(Capabilities.wgpu) is want, (K, N, block, nbytes)
