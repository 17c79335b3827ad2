"""GPU: sa_taps_unfold / sa_taps_fold (csrc/taps.hip) against the numpy loops of tests/taps_ref.py: unfold bit for bit in the three storage types with zeroed
padding columns and a bounded bias gradient, fold under the fp64 bound of tests/conv_bounds.py and bitwise reproducible, and the argument checks."""
import numpy as np
import pytest
import torch

import conv_bounds as cb
import taps_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
TUPLES = [(3, 2, 1, 1), (2, 2, 0, 1), (4, 2, 1, 1), (3, 1, 2, 2), (4, 1, 1, 1)]      # (k, s, p, d)
VOLUMES = [(9, 11, 13), (8, 10, 35)]
N = 2


def _unfold(x, dtype, grid, k, mult, step, off, ld, db=None):
    from synthanatomy_amd import _ffi
    n, D, H, W = x.shape
    Xc = torch.full((n, *grid, ld), float("nan"), dtype=dtype, device=DEV)
    rc = _ffi.lib().sa_taps_unfold(_ffi.ptr(x), _ffi.dtype_id(dtype), _ffi.ptr(Xc), _ffi.ptr(db), n, D, H, W, *grid, k, mult, step, off, ld, _ffi.stream())
    return rc, Xc


def _fold(P, bias, odims, k, s, p, d):
    from synthanatomy_amd import _ffi
    n, Dc, Hc, Wc, ld = P.shape
    out = torch.full((n, *odims), float("nan"), dtype=torch.float32, device=DEV)
    rc = _ffi.lib().sa_taps_fold(_ffi.ptr(P), _ffi.ptr(bias), _ffi.ptr(out), n, Dc, Hc, Wc, *odims, k, s, p, d, ld, _ffi.stream())
    return rc, out


@pytest.fixture(scope="module")
def volumes():
    gen = torch.Generator().manual_seed(11)
    return {v: torch.randn(N, *v, generator=gen) for v in VOLUMES}


@pytest.mark.parametrize("vol", VOLUMES, ids=str)
@pytest.mark.parametrize("tup", TUPLES, ids=str)
def test_unfold_bit_exact(tup, vol, volumes):
    from synthanatomy_amd import _ffi
    k, s, p, d = tup
    x = volumes[vol]
    grid = tuple(taps_ref.conv_out(i, k, s, p, d) for i in vol)
    xd = x.to(DEV)
    for dtype, vec in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float16, 8)):
        for ld in ((k ** 3 + vec - 1) // vec * vec, (k ** 3 + vec - 1) // vec * vec + vec):
            ref = torch.from_numpy(taps_ref.unfold(x.numpy(), grid, k, s, d, -p, ld)).to(dtype)
            db0 = torch.tensor([0.375])
            db = db0.to(DEV)
            with _ffi.kernel_log() as names:
                rc, Xc = _unfold(xd, dtype, grid, k, s, d, -p, ld, db)
                torch.cuda.synchronize()
            assert rc == 0, rc
            assert any(n.startswith("taps_unfold_kernel") for n in names), names
            got = Xc.cpu()
            assert not torch.isnan(got.float()).any()
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(got.view(bits), ref.view(bits)), f"{tup} {vol} {dtype} ld {ld}: {(got.float() != ref.float()).sum()} elements differ"
            assert not got[..., k ** 3:].any(), "padding columns"
            rdb = x.double().sum().reshape(1) + db0.double()
            Ab = x.double().abs().sum().reshape(1) + db0.double().abs()
            ok, ratio, _ = cb.check(db, rdb, Ab)
            assert ok, f"db: max|err|/A = {ratio:.2e}"
            # a db that forgets the last depth plane of the last image is out of bound
            assert not cb.check(db, rdb - x[-1, -1].double().sum(), Ab)[0]


@pytest.mark.parametrize("vol", VOLUMES, ids=str)
@pytest.mark.parametrize("tup", TUPLES, ids=str)
def test_fold_bounded_and_reproducible(tup, vol):
    from synthanatomy_amd import _ffi
    k, s, p, d = tup
    cells = tuple(taps_ref.conv_out(i, k, s, p, d) for i in vol)
    gen = torch.Generator().manual_seed(k * 100 + s * 10 + p + sum(vol))
    for op in (0, 1):
        if op >= max(s, d):
            continue
        odims = tuple(taps_ref.convT_out(c, k, s, p, op, d) for c in cells)
        ld = (k ** 3 + 3) // 4 * 4 + 4
        P = torch.randn(N, *cells, ld, generator=gen)          # (the padding columns hold values too: they must not be read)
        bias = torch.tensor([0.3])
        Pd, bd = P.to(DEV), bias.to(DEV)
        with _ffi.kernel_log() as names:
            rc, out = _fold(Pd, bd, odims, k, s, p, d)
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert any(n.startswith("taps_fold_kernel") for n in names), names
        b = float(bias[0])                                     # (the fp32 value the kernel reads)
        ref, A = (torch.from_numpy(a) for a in taps_ref.fold(P.numpy(), b, odims, k, s, p, d))
        wit, _ = taps_ref.fold(np.where(np.arange(ld) == k ** 3 - 1, 0.0, P.numpy()), b, odims, k, s, p, d)     # witness: the last tap dropped
        cb.assert_bounded(f"fold {tup} {vol} op {op}", out, ref, A, torch.from_numpy(wit))
        rc, again = _fold(Pd, bd, odims, k, s, p, d)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out.view(torch.int32), again.view(torch.int32))
        rc, nob = _fold(Pd, None, odims, k, s, p, d)
        ok, ratio, _ = cb.check(nob, ref - b, A - abs(b))
        assert rc == 0 and ok, ratio


def test_argument_checks():
    from synthanatomy_amd import _ffi
    x = torch.zeros(1, 4, 4, 4, device=DEV)
    assert _unfold(x, torch.float32, (2, 2, 2), 3, 2, 1, -1, 24)[0] == _ffi.SA_EINVAL            # ld < k^3
    assert _unfold(x, torch.bfloat16, (2, 2, 2), 3, 2, 1, -1, 28)[0] == _ffi.SA_EINVAL           # 56-byte rows
    assert _unfold(x, torch.float32, (2, 2, 2), 5, 2, 1, -1, 128)[0] == _ffi.SA_EUNSUPPORTED     # k = 5
    Xc = torch.zeros(1, 2, 2, 2, 28, device=DEV)
    lib = _ffi.lib()
    assert lib.sa_taps_unfold(None, 0, _ffi.ptr(Xc), None, 1, 4, 4, 4, 2, 2, 2, 3, 2, 1, -1, 28, _ffi.stream()) == _ffi.SA_EINVAL
    assert lib.sa_taps_unfold(_ffi.ptr(x), 7, _ffi.ptr(Xc), None, 1, 4, 4, 4, 2, 2, 2, 3, 2, 1, -1, 28, _ffi.stream()) == _ffi.SA_EUNSUPPORTED
    assert lib.sa_taps_unfold(_ffi.ptr(x), 0, _ffi.ptr(Xc), None, 1, 4, 4, 4, 2 ** 31 - 8, 1, 1, 3, 2, 1, -1, 28, _ffi.stream()) == _ffi.SA_EINVAL
    P = torch.zeros(1, 2, 2, 2, 28, device=DEV)
    assert _fold(P, None, (4, 4, 4), 3, 2, 1, 1)[0] == 0
    assert _fold(P, None, (4, 4, 4), 4, 2, 1, 1)[0] == _ffi.SA_EINVAL                            # ld 28 < 64
    assert _fold(P, None, (4, 4, 4), 3, 3, 1, 1)[0] == _ffi.SA_EUNSUPPORTED                      # stride 3
    assert _fold(P, None, (4, 4, 4), 5, 2, 1, 1)[0] == _ffi.SA_EUNSUPPORTED
    out = torch.zeros(1, 4, 4, 4, device=DEV)
    assert lib.sa_taps_fold(_ffi.ptr(P), None, None, 1, 2, 2, 2, 4, 4, 4, 3, 2, 1, 1, 28, _ffi.stream()) == _ffi.SA_EINVAL
    assert lib.sa_taps_fold(_ffi.ptr(P), None, _ffi.ptr(out), 1, 2, 2, 2, 2 ** 31 - 8, 1, 1, 3, 2, 1, 1, 28, _ffi.stream()) == _ffi.SA_EINVAL
    torch.cuda.synchronize()
