"""NumPy reference of the cross-spectra of every plane against a few reference planes
(``Solver.plane_cross_spectra``; csrc/include/channel/kernels.hpp YCrossArgs) on top of the oracle, and
the two-point correlations across planes that follow from them.

With ``e(kx, kz; y, y_r) = a(kx, kz, y) conj(b(kx, kz, y_r))`` of every stored element (all signed
retained kx, kz >= 0; weight 1 at kz = 0 and 2 at kz > 0, the mean line excluded, as ``spectra``):

  ckx[row, i, y, k]  = sum over the stored elements with |kx| = k of wgt (e if kx >= 0 else conj(e)),
                       the real part only at k = 0 (the -kz twin of a (0, kz) element has kx = 0 too)
  ckz[row, i, y, kz] = sum over the stored kx of wgt e

For real fields ``<a'(x + r_x, y, z) b'(x, y_r, z)> = Re sum_k ckx[k] exp(i k ax r_x)``, and likewise in z
with ``ckz``; the sum of ``Re ckx`` (or ``Re ckz``) over k is the covariance ``<a'(y) b'(y_r)>``.
"""
from __future__ import annotations

import numpy as np

from .budgets import plane_weights
from .oracle import OracleSolver

# row sets: (name, field of the first factor at y, field of the conjugated factor at y_r), fields in the
# order of OracleSolver.fields (u, v, w, omega_x, omega_y, omega_z)
CROSS_ROWS = {
    "velocity": (("uu", 0, 0), ("vv", 1, 1), ("ww", 2, 2), ("uv", 0, 1)),
    "shear": (("u_wz", 0, 5), ("v_wz", 1, 5), ("w_wx", 2, 3), ("wz_wz", 5, 5)),
}
# rows that change sign under the reflection y -> -y (v, omega_x and omega_z are odd)
ODD_ROWS = ("uv", "u_wz", "w_wx")
# the fields of a row's two factors, for the normalisation by rows of ``spectra.SPECTRA_ROWS``
ROW_FACTORS = {"uu": ("uu", "uu"), "vv": ("vv", "vv"), "ww": ("ww", "ww"), "uv": ("uu", "vv"),
               "u_wz": ("uu", "wzwz"), "v_wz": ("vv", "wzwz"), "w_wx": ("ww", "wxwx"), "wz_wz": ("wzwz", "wzwz")}
MAX_REFS = 16


def row_names(rows: str = "velocity") -> tuple:
    if rows not in CROSS_ROWS:
        raise ValueError(f"unknown row set {rows!r} (velocity, shear)")
    return tuple(r[0] for r in CROSS_ROWS[rows])


def check_refs(refs, NY: int) -> list:
    refs = [int(j) for j in refs]
    if not refs or len(refs) > MAX_REFS:
        raise ValueError(f"1 to {MAX_REFS} reference planes, not {len(refs)}")
    if len(set(refs)) != len(refs) or min(refs) < 0 or max(refs) >= NY:
        raise ValueError(f"reference planes {refs} must be distinct and in [0, {NY})")
    return refs


def plane_cross_spectra(o: OracleSolver, refs, rows: str = "velocity") -> dict:
    """``{"rows", "ref_planes", "ckx" [4, nref, NY, Kx + 1], "ckz" [4, nref, NY, nkz]}``, complex, of a
    prepared ``OracleSolver`` (this rank's lines in arrays of the global size; a distributed caller sums
    over the ranks)."""
    names = row_names(rows)
    if o.fields is None:
        o.prepare()
    p = o.plan
    refs = check_refs(refs, p.NY)
    F = [o.lines(f) for f in o.fields]
    wgt = plane_weights(o)
    kx = np.asarray(p.kx_of(p.kx0 + np.arange(p.nkx_loc)))
    akx = np.abs(kx)
    ckx = np.zeros((4, len(refs), p.NY, p.Kx + 1), complex)
    ckz = np.zeros((4, len(refs), p.NY, p.nkz), complex)
    for q, (_, fa, fb) in enumerate(CROSS_ROWS[rows]):
        for i, yr in enumerate(refs):
            # (the weight is applied by selection: the mean line holds U and -U', not a fluctuation)
            e = np.where(wgt > 0, F[fa] * np.conj(F[fb][yr]), 0.0) * wgt
            e = e.reshape(p.NY, p.nkx_loc, p.nkz_loc)
            ckz[q, i, :, p.kz0:p.kz0 + p.nkz_loc] = e.sum(axis=1)
            ex = np.where((kx >= 0)[None, :, None], e, np.conj(e)).sum(axis=2)
            ex[:, kx == 0] = ex[:, kx == 0].real
            np.add.at(ckx[q, i], (slice(None), akx), ex)
    return {"rows": names, "ref_planes": refs, "ckx": ckx, "ckz": ckz}


def cross_correlations(c: np.ndarray, n: int) -> np.ndarray:
    """The real correlation ``Re sum_k c[..., k] exp(2 pi i k r / n)`` at the signed separations
    r = -n/2 .. n/2 - 1 grid intervals of a periodic direction of ``n`` points, from the complex bins
    k = 0 .. nk - 1 (nk - 1 <= n / 2): [..., nk] -> [..., n]."""
    c = np.asarray(c, complex)
    nk = c.shape[-1]
    if 2 * (nk - 1) > n:
        raise ValueError(f"{nk} bins do not fit a direction of {n} points")
    r = np.arange(n) - n // 2
    ph = np.exp(2j * np.pi * np.outer(np.arange(nk), r) / n)
    return (c @ ph).real
