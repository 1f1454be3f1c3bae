"""NumPy reference of the one-dimensional spectra and co-spectra at every plane
(``Solver.plane_spectra``; csrc/include/channel/kernels.hpp YSpectraArgs) on top of the oracle, and
the two-point correlations that follow from them.

Conventions (those of ``budgets`` and of the device kernels): fluctuations exclude the mean line
(kx = 0, kz = 0); a retained (kx, kz) counts once for kz = 0 and twice for kz > 0 (its -kz half);
+kx and -kx share the bin |kx|.  So summing a row over its wavenumber gives the plane mean of the
product: ``ekx.sum(-1) == ekz.sum(-1) == <a'b'>(y)``.
"""
from __future__ import annotations

import numpy as np

from .budgets import plane_weights
from .oracle import OracleSolver

SPECTRA_ROWS = ("uu", "vv", "ww", "uv", "wxwx", "wywy", "wzwz", "pp")
# rows whose spectrum is a power spectrum (the co-spectrum uv has no correlation coefficient)
AUTO_ROWS = ("uu", "vv", "ww", "wxwx", "wywy", "wzwz", "pp")


def plane_spectra(o: OracleSolver, p_hat: np.ndarray | None = None) -> dict:
    """``{"rows", "ekx" [8, NY, Kx + 1], "ekz" [8, NY, nkz]}`` of a prepared ``OracleSolver`` (this
    rank's lines in arrays of the global size; a distributed caller sums over the ranks).  ``p_hat``:
    the fluctuating static pressure [NY, nkx_loc, nkz_loc] for row ``pp`` (zero without it)."""
    if o.fields is None:
        o.prepare()
    p = o.plan
    u, v, w, wx, wy, wz = (o.lines(f) for f in o.fields)
    sq = lambda a: a.real ** 2 + a.imag ** 2  # noqa: E731
    rows = [sq(u), sq(v), sq(w), u.real * v.real + u.imag * v.imag, sq(wx), sq(wy), sq(wz)]
    rows.append(sq(np.asarray(p_hat, complex).reshape(p.NY, -1)) if p_hat is not None else np.zeros_like(rows[0]))
    # (the weight is applied by selection: the mean line of u and omega_z holds U and -U', not a fluctuation)
    wgt = plane_weights(o)
    prod = np.where(wgt > 0, np.stack(rows), 0.0) * wgt          # [8, NY, lines]
    prod = prod.reshape(len(rows), p.NY, p.nkx_loc, p.nkz_loc)
    ekx = np.zeros((len(rows), p.NY, p.Kx + 1))
    ekz = np.zeros((len(rows), p.NY, p.nkz))
    akx = np.abs(p.kx_of(p.kx0 + np.arange(p.nkx_loc)))
    np.add.at(ekx, (slice(None), slice(None), akx), prod.sum(axis=3))
    ekz[:, :, p.kz0:p.kz0 + p.nkz_loc] = prod.sum(axis=2)
    return {"rows": SPECTRA_ROWS, "ekx": ekx, "ekz": ekz}


def correlations(e: np.ndarray, n: int) -> np.ndarray:
    """Two-point correlation coefficient at the separations 0 .. n // 2 grid intervals from the
    one-sided spectrum ``e`` [..., nk] (bins k = 0 .. nk - 1 of a periodic direction of ``n`` points,
    nk - 1 <= n / 2): R(r) = sum_k e(k) cos(2 pi k r / n) / sum_k e(k).  Where the spectrum sums to
    zero (the walls) the result is 0."""
    e = np.asarray(e, float)
    nk = e.shape[-1]
    if 2 * (nk - 1) > n:
        raise ValueError(f"{nk} bins do not fit a direction of {n} points")
    c = np.cos(2.0 * np.pi * np.outer(np.arange(nk), np.arange(n // 2 + 1)) / n)
    r = e @ c
    r0 = r[..., :1]
    ok = r0 != 0
    return np.where(ok, r / np.where(ok, r0, 1.0), 0.0)
