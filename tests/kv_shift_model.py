"""The context shift of a KV lane (zgml_amd/csrc/kv_shift.h) restated in numpy, shared by tests/test_kv_shift_host.py (the header
against this model, to the bit) and tests/test_hip_kv_shift.py (the kernel against this model, to the bit).

Every product and every sum is a float32 numpy operation, so each is rounded to f32 on its own, as the rule demands. Lanes are
arrays [n_cols, d_head]; an int8 lane is (int8 [n_cols, d_head], float32 scales [n_cols, d_head / 32])."""
import numpy as np

f32 = np.float32


def shift_rows(cos, sin, discard):
    """(c, s): the first half of row `discard` of the model's [max_seq, d_head] tables"""
    hd = cos.shape[1] // 2
    return np.ascontiguousarray(cos[discard, :hd], f32), np.ascontiguousarray(sin[discard, :hd], f32)


def rotate(cols, c, s):
    """cols [n, d_head] f32 -> the columns turned back by the rows' angle: lo' = fl(fl(lo c) + fl(hi s)), hi' = fl(fl(hi c) - fl(lo s))"""
    cols = np.asarray(cols, f32)
    hd = cols.shape[-1] // 2
    lo, hi = cols[..., :hd], cols[..., hd:]
    c, s = np.asarray(c, f32), np.asarray(s, f32)
    with np.errstate(all="ignore"):
        out_lo = (lo * c).astype(f32) + (hi * s).astype(f32)
        out_hi = (hi * c).astype(f32) - (lo * s).astype(f32)
    return np.concatenate([out_lo, out_hi], axis=-1).astype(f32)


def quantise(cols):
    """kvq.h's column rule: cols [n, d_head] f32 -> (int8 [n, d_head], f32 scales [n, d_head / 32])"""
    cols = np.asarray(cols, f32)
    n, dh = cols.shape
    blocks = cols.reshape(n, dh // 32, 32)
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(np.abs(blocks), axis=2, initial=f32(0))  # (fmaxf: a NaN operand is ignored)
        pos = mx > 0
        safe = np.where(pos, mx, f32(1))
        scale = np.where(pos, safe / f32(127), f32(1)).astype(f32)
        inv = np.where(pos, f32(127) / safe, f32(0)).astype(f32)
        scaled = (blocks * inv[:, :, None]).astype(f32)
        q = np.fmax(f32(-127), np.fmin(scaled, f32(127)))  # (the reference's clamp: min, then max, each keeping the operand that is a number)
    return np.trunc(q).astype(np.int8).reshape(n, dh), scale


def dequantise(q, scales):
    n, dh = q.shape
    return (q.astype(f32).reshape(n, dh // 32, 32) * scales.astype(f32)[:, :, None]).astype(f32).reshape(n, dh)


def shift_f32(lane, keep, discard, n_filled, is_k, c=None, s=None):
    """-> the shifted copy of lane [n_cols, d_head]: columns [keep + discard, n_filled) at [keep, n_filled - discard), K columns
    rotated; everything else as it was"""
    out = np.array(lane, f32, copy=True)
    if discard == 0 or keep + discard >= n_filled:
        return out
    moved = lane[keep + discard:n_filled]
    out[keep:n_filled - discard] = rotate(moved, c, s) if is_k else moved
    return out


def shift_i8(q, scales, keep, discard, n_filled, is_k, c=None, s=None):
    """-> (q, scales) shifted: a moved K column is dequantised, rotated and requantised as a whole; a V column's bytes and scales move"""
    q2, sc2 = np.array(q, np.int8, copy=True), np.array(scales, f32, copy=True)
    if discard == 0 or keep + discard >= n_filled:
        return q2, sc2
    mq, ms = q[keep + discard:n_filled], scales[keep + discard:n_filled]
    if is_k:
        mq, ms = quantise(rotate(dequantise(mq, ms), c, s))
    q2[keep:n_filled - discard], sc2[keep:n_filled - discard] = mq, ms
    return q2, sc2


# ── cache images (include/zgml_hip.h: the quantised cache layout) ──
def split_cache(img, n_cols, dh):
    """f32 image of an int8 cache -> (int8 [n_cols, dh] view, f32 scales [n_cols, dh / 32] view)"""
    nq = n_cols * dh // 4
    return img[:nq].view(np.int8).reshape(n_cols, dh), img[nq:nq + n_cols * (dh // 32)].reshape(n_cols, dh // 32)


def shift_cache_image(img, n_cols, dh, keep, discard, n_filled, is_k, c=None, s=None):
    """the shift applied to an int8 cache image in place (img may be longer than the cache: the rest is untouched)"""
    q, sc = split_cache(img, n_cols, dh)
    q2, sc2 = shift_i8(q, sc, keep, discard, n_filled, is_k, c, s)
    q[:], sc[:] = q2, sc2
    return img
