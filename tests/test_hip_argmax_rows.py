"""The greedy pick on the MI355X at the sizes where its shape changes (Backend.argmax -> launch_argmax; kernels:
zgml_amd/csrc/greedy_tail.hip over the shared scan / reduction bodies of zgml_amd/csrc/tail_device.h).

A row of n values takes n // 1024 + 1 workgroups of 256 threads, at most 256, so a thread walks up to four elements, a grid of
threads apart, below the cap and more beyond it: the sizes straddle one thread, one workgroup, several workgroups, the size at
which the 256-workgroup cap is reached (261120) and one beyond it, where the walk grows past four. The expected value is
numpy.argmax over the same slice — first maximum wins, the kernels' rule and the oracle's for NaN-free input — compared by exact
equality. No NaNs: where a NaN lands in the strided walk
decides the result, and that is not a contract."""
import numpy as np
import pytest

from tests.test_hip_logprob import upload

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, 65537, 261119, 261120, 262147)


def planted(n, at):
    """seeded normal values with the maximum planted at every index of `at` that exists"""
    v = np.random.default_rng(n).standard_normal(n).astype(f32)
    top = f32(v.max() + 1.0)
    for i in at:
        if 0 <= i < n:
            v[i] = top
    return v


def patterns(n):
    yield "max at 0 and n-1", planted(n, (0, n - 1))
    yield "max at n//2 and n//2+1", planted(n, (n // 2, n // 2 + 1))
    yield "all equal", np.full(n, 0.25, f32)
    yield "all -inf", np.full(n, -np.inf, f32)
    yield "strictly increasing", np.arange(n, dtype=f32)  # (exact below 2^24)
    v = np.zeros(n, f32)
    v[0] = -0.0
    yield "-0.0 then +0.0", v


@pytest.mark.parametrize("n", SIZES)
def test_argmax_first_maximum_wins(hip_backend, n):
    for name, v in patterns(n):
        h = upload(hip_backend, v)
        got = hip_backend.argmax(h, 0, 0, n)
        hip_backend.freeProgram(h)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert got == int(np.argmax(v)), (name, n)


def test_argmax_of_a_slice_at_an_odd_offset(hip_backend):
    offset, n = 101, SIZES[-1]
    for at in ((0, n - 1), (offset - 1, offset, n - 1), (n // 2, n // 2 + 1)):  # (a maximum in front of the slice is not its)
        v = planted(n, at)
        h = upload(hip_backend, v)
        got = hip_backend.argmax(h, 0, offset, n - offset)
        hip_backend.freeProgram(h)
        assert not hip_backend.last_error(), hip_backend.last_error()
        assert got == int(np.argmax(v[offset:])), at
