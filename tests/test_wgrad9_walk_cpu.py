"""CPU: the step walk of the nine-tap 3x3x3 weight-gradient kernel (csrc/conv_wgrad.hip: Wgrad9Walk).  The kernel decomposes a block's first
step index once and then carries (wp, hq, d, n) from step to step instead of dividing; sa_wgrad9_step_walk runs that very helper on the host.
Every step of the test shapes of tests/test_wgrad9_schedule_gpu.py and of the two production launches (batch 8, 80x112x80 and 40x56x40) must
carry to what the division gives, from the start and from block starts inside the range."""
import ctypes

import pytest

SHAPES = [(1, (3, 8, 16)), (2, (5, 9, 17)), (1, (4, 16, 40)), (2, (65, 15, 31)), (1, (86, 16, 40)), (8, (80, 112, 80)), (8, (40, 56, 40))]


def _lib():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    fn = lib.sa_wgrad9_step_walk
    fn.restype, fn.argtypes = _ffi._SIGS["sa_wgrad9_step_walk"]
    return fn


@pytest.mark.parametrize("N,dims", SHAPES, ids=[f"{n}x{'x'.join(map(str, d))}" for n, d in SHAPES])
def test_carried_counters_equal_the_division(N, dims):
    fn = _lib()
    D, H, W = dims
    HQ, WP = -(-H // 8), -(-W // 16)
    nsteps = N * D * HQ * WP
    starts = sorted({0, 1, min(17, nsteps - 1), nsteps // 3, nsteps // 2 + 1, max(0, nsteps - 5), nsteps - 1})
    for step0 in starts:
        count = nsteps - step0
        out = (ctypes.c_uint32 * (4 * count))()
        assert fn(WP, HQ, D, step0, count, out) == 0
        for i in range(count):
            q1, wp = divmod(step0 + i, WP)
            q2, hq = divmod(q1, HQ)
            n, d = divmod(q2, D)
            assert tuple(out[4 * i:4 * i + 4]) == (wp, hq, d, n), (step0, i)
        assert out[4 * (count - 1) + 3] == N - 1      # the last step lies in the last image


def test_the_entry_refuses_a_zero_extent():
    fn = _lib()
    out = (ctypes.c_uint32 * 4)()
    assert fn(0, 1, 1, 0, 1, out) != 0 and fn(1, 0, 1, 0, 1, out) != 0 and fn(1, 1, 0, 0, 1, out) != 0 and fn(1, 1, 1, 0, 1, None) != 0
