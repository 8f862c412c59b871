"""A float64 numpy model of the sampling rule of include/zgml_hip.h (zgml_sampling), written from the contract's text and sharing
no code with zgml_amd/csrc/sample.h: np.exp, cumsum, searchsorted. tests/test_sample_host.py runs the header (through
tests/cpp/sample_probe.cpp) against it.

The header sums in f32 and the model in f64, so a threshold that falls next to a prefix sum may legitimately land on either side
of it. `pick` therefore also says whether a case is AMBIGUOUS, by the model's numbers alone:
  * u * cum_m lies within MARGIN * cum_m of a prefix sum, or
  * top_p < 1 and top_p * total lies within MARGIN * total of a prefix sum.
Nothing else may set a case aside."""
import numpy as np

MARGIN = 1e-5
MAX_K = 256


def candidates(v, top_k):
    """indices of the k = min(top_k or 256, n) largest logits: value descending, the lower index first among equals; -0 == +0,
    a NaN counts as -inf"""
    v = np.asarray(v, np.float32).astype(np.float64)
    v = np.where(np.isnan(v), -np.inf, v) + 0.0
    order = np.lexsort((np.arange(v.size), -v))  # (the last key is the primary one)
    return order[:min(top_k or MAX_K, MAX_K, v.size)]


def pick(values, temperature, top_p, u):
    """values: the candidates' logits in candidate order. -> (rank of the sampled candidate, ambiguous)"""
    v = np.asarray(values, np.float64)
    inv_t = float(np.float32(1.0) / np.float32(temperature))  # (the contract's f32 reciprocal, computed once)
    d = (v - v[0]) * inv_t
    p = np.where(d >= -87.0, np.exp(d), 0.0)
    cum = np.cumsum(p)
    total = cum[-1]
    ambiguous = False
    m = v.size
    if top_p < 1.0:
        thr = float(np.float32(top_p)) * total
        m = min(int(np.searchsorted(cum, thr, side="left")) + 1, v.size)  # the smallest prefix whose sum is >= thr
        ambiguous |= bool(np.any(np.abs(cum - thr) <= MARGIN * total))
    cum_m = cum[m - 1]
    t = u * cum_m
    j = int(np.searchsorted(cum[:m], t, side="right"))  # the first running sum > t
    ambiguous |= bool(np.any(np.abs(cum[:m] - t) <= MARGIN * cum_m))
    return min(j, m - 1), ambiguous
