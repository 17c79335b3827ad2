"""fp64 restatement, in torch, of the half-spectrum formulas behind ``sa_fourier_loss`` (csrc/spectral.hip) for the reference's ``SpectralLoss``,
``HartleyLoss`` and ``WaveGANLoss`` (src/losses/vqvae/vqvae.py:188-323, 326-519, 641-771), pixel and quantization terms included.

Y = the ortho rfftn over (C, D, H, W) of the float64 volumes, with Im forced to +0 on the self-conjugate bins (every transformed index 0 or m/2);
m = the bin's multiplicity along W.  The value is the full-spectrum sum written on the half spectrum; d loss / d pred is irfftn of the Hermitian half
of the spectrum-domain gradient G (imaginary part 0 on the self-conjugate bins).  Where |Yp| = 0 the unit phasor is taken as 0.

Each function returns ``(loss, summaries, d loss / d pred)``; summaries use the reference's keys (without the quantization entries).
"""
import torch

DIMS = (1, 2, 3, 4)


def _spectra(x, y):
    C, D, H, W = x.shape[1:]
    Yp, Yy = (torch.fft.rfftn(t.double(), dim=DIMS, norm="ortho") for t in (x, y))
    dev = Yp.device

    def edge(m, k):
        i = torch.arange(k, device=dev)
        return (i == 0) | (2 * i == m)

    kw = edge(W, W // 2 + 1)
    sc = edge(C, C)[:, None, None, None] & edge(D, D)[:, None, None] & edge(H, H)[:, None] & kw
    Yp = torch.complex(Yp.real, torch.where(sc, torch.zeros_like(Yp.imag), Yp.imag))
    Yy = torch.complex(Yy.real, torch.where(sc, torch.zeros_like(Yy.imag), Yy.imag))
    mult = torch.where(kw, 1.0, 2.0).double()
    return Yp, Yy, mult, sc


def _to_pred(G, sc, shape):
    G = torch.complex(G.real, torch.where(sc, torch.zeros_like(G.imag), G.imag))
    return torch.fft.irfftn(G, s=tuple(shape[1:]), dim=DIMS, norm="ortho")


def _unit(Yp, Ap):
    return torch.where(Ap > 0, Yp / torch.where(Ap > 0, Ap, 1.0), torch.zeros_like(Yp))


def _finish(spec, grad, pred, y, q, include_pixel_loss, summ):
    loss = spec
    if include_pixel_loss:
        d = pred.double() - y.double()
        l2 = (d * d).mean()
        summ["Loss-MSE-Reconstruction"] = l2
        loss = loss + l2
        grad = grad + 2 * d / d.numel()
    for ql in q:
        loss = loss + float(ql)
    return loss, summ, grad


def spectral(pred, y, q=(), fft_factor=1.0, include_pixel_loss=True):
    Yp, Yy, m, sc = _spectra(pred, y)
    n = pred.numel()
    Ap, Ay = Yp.abs(), Yy.abs()
    dphi = torch.angle(Yp) - torch.angle(Yy)
    e = torch.exp(dphi.abs())
    amp = 0.5 / n * (m * (Ap - Ay) ** 2).sum()
    phase = 0.5 / n * (m * (1 - e) ** 2).sum()
    spec = (amp + phase) * fft_factor
    u = _unit(Yp, Ap)
    gphi = torch.where(Ap > 0, (e - 1) * e * torch.sign(dphi) / (n * torch.where(Ap > 0, Ap, 1.0)), 0.0)
    G = fft_factor * ((Ap - Ay) / n * u + gphi * 1j * u)
    summ = {"Loss-Amplitude-Reconstruction": amp, "Loss-Phase-Reconstruction": phase, "Loss-Spectral-Reconstruction": spec}
    return _finish(spec, _to_pred(G, sc, pred.shape), pred, y, q, include_pixel_loss, summ)


def hartley_weight(D, H, W, device=None):
    """The reference's high-frequency weight on the half spectrum [D, H, W // 2 + 1] (separable min / max, no table of the full volume)."""
    def axis(mm, k):
        i = torch.arange(k, dtype=torch.float64, device=device)
        t = ((mm / 2 - i).abs() / (mm / 2)) ** 2
        full = ((mm / 2 - torch.arange(mm, dtype=torch.float64, device=device)).abs() / (mm / 2)) ** 2
        return t, full.min(), full.max()

    (td, lo_d, hi_d), (th, lo_h, hi_h), (tw, lo_w, hi_w) = axis(D, D), axis(H, H), axis(W, W // 2 + 1)
    q = td[:, None, None] + th[None, :, None] + tw[None, None, :]
    emin, emax = torch.exp(lo_d + lo_h + lo_w), torch.exp(hi_d + hi_h + hi_w)
    return (torch.exp(q) - emin) / (emax - emin) + 1e-4


def hartley(pred, y, q=(), fht_factor=1.0, include_pixel_loss=True, prioritise_high_frequency=True):
    Yp, Yy, m, sc = _spectra(pred, y)
    n = pred.numel()
    w2 = hartley_weight(*pred.shape[2:], device=pred.device) ** 2 if prioritise_high_frequency else torch.ones((), dtype=torch.float64)
    diff = Yp - Yy
    spec = fht_factor * 0.5 / n * (m * w2 * diff.abs() ** 2).sum()
    G = fht_factor * w2 * diff / n
    summ = {"Loss-Hartley-Reconstruction": spec}
    return _finish(spec, _to_pred(G, sc, pred.shape), pred, y, q, include_pixel_loss, summ)


def wavegan(pred, y, q=(), fft_factor=1.0, include_pixel_loss=True):
    Yp, Yy, m, sc = _spectra(pred, y)
    n = pred.numel()
    Ap, Ay = Yp.abs(), Yy.abs()
    S, N = torch.sqrt((m * (Ay - Ap) ** 2).sum()), torch.sqrt((m * Ay ** 2).sum())
    dl = torch.log(Ay) - torch.log(Ap)
    l_sc, l_mag = S / N, (m * dl.abs()).sum() / n
    spec = (l_sc + l_mag) * fft_factor
    ga = (Ap - Ay) / (S * N) - torch.sign(dl) / (n * torch.where(Ap > 0, Ap, 1.0))
    G = fft_factor * ga * _unit(Yp, Ap)
    summ = {"Loss-Spectral_Convergence-Reconstruction": l_sc, "Loss-Log_Magnitude-Reconstruction": l_mag, "Loss-Spectral-Reconstruction": spec}
    return _finish(spec, _to_pred(G, sc, pred.shape), pred, y, q, include_pixel_loss, summ)


def by_name(name, pred, y, q=(), factor=1.0, include_pixel_loss=True):
    """``name``: spectral, hartley, hartley_flat (prioritise_high_frequency=False) or wavegan, as the golden cases are named."""
    if name == "spectral":
        return spectral(pred, y, q, factor, include_pixel_loss)
    if name in ("hartley", "hartley_flat"):
        return hartley(pred, y, q, factor, include_pixel_loss, prioritise_high_frequency=name == "hartley")
    if name == "wavegan":
        return wavegan(pred, y, q, factor, include_pixel_loss)
    raise ValueError(name)


def reference_way_fp32(name, pred, y):
    """The spectral term and its gradient composed as the reference writes them, in the volumes' own dtype (fp32): full complex ortho fftn over
    dims (1, 2, 3, 4), amplitudes / phases / Hartley transform, autograd.  The yardstick for how close an fp32 computation of the same loss gets
    to :func:`by_name` (fp64): the phase term is ill-conditioned where |Y| is small or Y lies near the negative real axis."""
    p = pred.detach().clone().requires_grad_(True)
    fp, fy = torch.fft.fftn(p, dim=DIMS, norm="ortho"), torch.fft.fftn(y, dim=DIMS, norm="ortho")
    if name in ("hartley", "hartley_flat"):
        hp, hy = fp.real - fp.imag, fy.real - fy.imag
        if name == "hartley":
            D, H, W = pred.shape[2:]
            td, th, tw = ((((m / 2 - torch.arange(m, dtype=torch.float64, device=pred.device)).abs() / (m / 2)) ** 2) for m in (D, H, W))
            w = torch.exp(td[:, None, None] + th[None, :, None] + tw[None, None, :])
            w = (w - w.min()) / (w - w.min()).max() + 1e-4
            hp, hy = hp * w, hy * w
        loss = 0.5 * torch.nn.functional.mse_loss(hp, hy)
    else:
        ap, ay = torch.sqrt(fp.real ** 2 + fp.imag ** 2), torch.sqrt(fy.real ** 2 + fy.imag ** 2)
        if name == "spectral":
            phase = torch.mean(0.5 * torch.abs((1 - torch.exp(torch.abs(torch.atan2(fp.imag, fp.real) - torch.atan2(fy.imag, fy.real)))) ** 2))
            loss = 0.5 * torch.nn.functional.mse_loss(ap, ay) + phase
        else:
            loss = torch.norm(ay - ap, p="fro") / torch.norm(ay, p="fro") + torch.nn.functional.l1_loss(torch.log(ay), torch.log(ap))
    (grad,) = torch.autograd.grad(loss, p)
    return loss.detach(), grad
