"""Host side of the Chebyshev recurrence (HxvSector.chebyshev_moments / chebyshev_apply and their _real forms, include/hxv.h): the spectral
window, the coefficient series of e^{-tau H} and e^{-iHt}, thermal typical states from a seeded device vector, the Jackson kernel and the
kernel-polynomial reconstruction of a spectral function.

Conventions.  The window (a, b) maps the spectrum into [-1, 1]:  x = (E - b)/a,  a > 0,  spectrum of H inside [b - a, b + a].  A series
f(E) = sum_n c_n T_n(x) is what chebyshev_apply takes as `coef`.  numpy only: the Bessel values come from this module's own backward
(Miller) recurrences."""
from __future__ import annotations

import numpy as np


def spectral_window(sec, nlanc: int = 60, margin: float = 0.02):
    """(a, b) for an open sector: the extremal Ritz values of ONE short lanczos_tridiag run on the engine's deterministic start vector,
    widened by `margin` of the window's width on EACH side.  Ritz values lie inside the spectrum, so without the margin the window is too
    narrow by construction; 60 steps put the extremal ones within ~1e-3 of the width on the models here, and the margin covers the rest.
    A miss is caught by the driver's guard (HxvError: spectrum outside the window), not silently: widen the margin then.  Collective on a
    split sector (every rank gets the same numbers)."""
    from .distributed import start_vector_slab

    nlanc = max(2, min(int(nlanc), int(sec.Dim)))
    v = start_vector_slab(sec.DimUp, sec.mpiQdw, sec.mpiIshift // max(sec.DimUp, 1), sec.pitch, sec._dev())
    al, bl, n = sec.lanczos_tridiag(v, nlanc)
    T = np.diag(al[:n]) + np.diag(bl[1:n], 1) + np.diag(bl[1:n], -1)
    ritz = np.linalg.eigvalsh(T)
    lo, hi = float(ritz[0]), float(ritz[-1])
    width = max(hi - lo, 1e-12 * max(abs(lo), abs(hi), 1.0))
    lo, hi = lo - margin * width, hi + margin * width
    return 0.5 * (hi - lo), 0.5 * (hi + lo)


def _miller_start(z: float) -> int:
    """An order far enough above z that both J_n(z) and e^{-z} I_n(z) are below 1e-30 of their largest value there and beyond."""
    return int(1.2 * z + 20.0 * z ** (1.0 / 3.0) + 60.0)


def _miller(z: float, sign: float):
    """y_n, n = 0 .. N, of the backward recurrence  y_{n-1} = (2n/z) y_n + sign * y_{n+1}  started from y_{N+1} = 0, y_N = tiny, rescaled on
    the way so that nothing overflows; un-normalised."""
    N = _miller_start(z)
    y = np.zeros(N + 2)
    y[N] = 1e-300
    for n in range(N, 0, -1):
        y[n - 1] = (2.0 * n / z) * y[n] + sign * y[n + 1]
        if abs(y[n - 1]) > 1e250:
            y[n - 1:] *= 1e-250
    return y[: N + 1]


def bessel_j(z: float):
    """J_n(z) for n = 0 .. N(z), N far past the last one above 1e-30: Miller's backward recurrence J_{n-1} = (2n/z) J_n - J_{n+1}, normalised
    with  1 = J_0 + 2 sum_{k>=1} J_{2k}.  z real; J_n(-z) = (-1)^n J_n(z)."""
    z = float(z)
    if z == 0.0:
        return np.array([1.0])
    y = _miller(abs(z), -1.0)
    y /= y[0] + 2.0 * y[2::2].sum()
    if z < 0.0:
        y[1::2] *= -1.0
    return y


def bessel_ie(z: float):
    """e^{-|z|} I_n(z) for n = 0 .. N(z) (the exponentially scaled modified Bessel function, scipy's ive): backward recurrence
    I_{n-1} = (2n/z) I_n + I_{n+1}, normalised with  e^{z} = I_0 + 2 sum_{n>=1} I_n.  z real; I_n(-z) = (-1)^n I_n(z)."""
    z = float(z)
    if z == 0.0:
        return np.array([1.0])
    y = _miller(abs(z), 1.0)
    y /= y[0] + 2.0 * y[1:].sum()
    if z < 0.0:
        y[1::2] *= -1.0
    return y


def _truncate(c: np.ndarray, tol: float) -> np.ndarray:
    """c up to the first order from which the tail sum_{n >= K} |c_n| stays below tol * max|c| (at least one term)."""
    mag = np.abs(c)
    tail = np.cumsum(mag[::-1])[::-1]
    keep = np.nonzero(tail >= tol * mag.max())[0]
    return c[: max(int(keep[-1]) + 1 if keep.size else 1, 1)]


def exp_coefficients(tau: float, a: float, b: float, tol: float = 1e-14) -> np.ndarray:
    """c_n with  e^{-tau E} = sum_n c_n T_n((E - b)/a)  on the window, tau real:  e^{-tau E} = e^{-b tau} e^{-(a tau) x}  and
    e^{-z x} = I_0(z) + 2 sum_{n>=1} (-1)^n I_n(z) T_n(x),  so  c_n = e^{-b tau + |a tau|} (2 - delta_n0) (-1)^n [e^{-|z|} I_n(z)],  z = a tau.
    The prefactor is the function's largest value on the window; the series stops where the tail of the scaled terms falls below tol."""
    z = float(a) * float(tau)
    y = bessel_ie(-z)  # I_n(-z) = (-1)^n I_n(z)
    c = 2.0 * y
    c[0] = y[0]
    return (_truncate(c, tol) * np.exp(-float(b) * float(tau) + abs(z))).astype(np.complex128)


def propagator_coefficients(t: float, a: float, b: float, tol: float = 1e-14) -> np.ndarray:
    """c_n with  e^{-i E t} = sum_n c_n T_n((E - b)/a):  e^{-i z x} = J_0(z) + 2 sum_{n>=1} (-i)^n J_n(z) T_n(x),  z = a t, times e^{-i b t}.
    The series stops where the tail falls below tol (the function has modulus 1)."""
    z = float(a) * float(t)
    y = bessel_j(z)
    c = 2.0 * y * np.array([1.0, -1j, -1.0, 1j])[np.arange(y.size) % 4]  # (-i)^n, exactly
    c[0] = y[0]
    return _truncate(c, tol) * np.exp(-1j * float(b) * float(t))


def thermal_state(sec, beta: float, a: float, b: float, seed: int, real: bool | None = None, tol: float = 1e-14):
    """A thermal typical state  e^{-beta H/2}|r>  of an open sector, entirely on the device: |r> = sec.random_vector(seed) (real-valued on the
    real path, complex-valued otherwise), the series exp_coefficients(beta/2, a, b, tol) and one chebyshev_apply[_real].  (a, b): a window
    around the spectrum (spectral_window).  real = None takes the real-vector path where sec.real_vectors_available; real = True on a sector
    without real vectors raises; real = False runs on complex vectors.  -> (out, norm2 = <out|out>), out in the padded layout.  Collective
    on a split sector."""
    from .engine import HxvError

    if real is None:
        real = bool(sec.real_vectors_available)
    elif real and not sec.real_vectors_available:
        raise HxvError("thermal_state(real=True): real vectors are not available on this sector (complex amplitudes, the spH0nd block or debug options)")
    r = sec.random_vector(seed, complex_valued=not real)
    coef = exp_coefficients(0.5 * float(beta), a, b, tol)
    if real:
        return sec.chebyshev_apply_real(r, coef.real, a, b)
    return sec.chebyshev_apply(r, coef, a, b)


def jackson(N: int) -> np.ndarray:
    """The Jackson damping factors g_n, n < N, of a series of N moments:
    g_n = [(N - n + 1) cos(pi n/(N+1)) + sin(pi n/(N+1)) cot(pi/(N+1))] / (N + 1)."""
    n = np.arange(N, dtype=np.float64)
    q = np.pi / (N + 1)
    return ((N - n + 1) * np.cos(q * n) + np.sin(q * n) / np.tan(q)) / (N + 1)


def spectral_function(moments, a: float, b: float, omega, kernel: str | None = "jackson") -> np.ndarray:
    """The kernel-polynomial reconstruction on the frequencies `omega`:
        A(w) = [g_0 mu_0 + 2 sum_{n>=1} g_n mu_n T_n(x)] / (pi a sqrt(1 - x^2)),   x = (w - b)/a,
    zero outside the window.  moments: mu_n along the first axis -- chebyshev_moments' self_moments (real) or its moments array
    [nmom, nprobes] (complex; one curve per probe, returned as [len(omega), nprobes]).  kernel: "jackson" or None (g_n = 1, the bare
    truncated series).  The resolution is uniform in arccos x: pi/N, i.e. about pi a / N in energy at the centre of the window."""
    mu = np.asarray(moments)
    N = mu.shape[0]
    if kernel == "jackson":
        g = jackson(N)
    elif kernel is None or kernel == "none":
        g = np.ones(N)
    else:
        raise ValueError("kernel must be 'jackson' or None")
    w = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    x = (w - b) / a
    inside = np.abs(x) < 1.0
    th = np.arccos(np.where(inside, x, 0.0))
    eps = np.full(N, 2.0)
    eps[0] = 1.0
    tn = np.cos(np.outer(th, np.arange(N))) * (g * eps)  # [nw, N]
    dens = tn @ mu.reshape(N, -1)
    dens = dens / (np.pi * a * np.sqrt(np.where(inside, 1.0 - x * x, 1.0)))[:, None]
    dens[~inside] = 0.0
    return dens.reshape((w.size,) + mu.shape[1:])
