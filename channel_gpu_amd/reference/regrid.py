"""NumPy fp64 reference of restarting on another grid (README "Restarting on another grid").

Written from the semantics, independently of csrc/core/regrid.cpp:

* x and z: target signed kx = k (|k| <= NX_d // 3) takes the source's k if |k| <= NX_s // 3, target
  kz takes the source's kz if kz <= (2 NZ_s - 2) // 3; every other target mode is zero.
* y: Lagrange interpolation in the physical coordinate on the source's tanh grid over a contiguous
  stencil of W = min(width, NY_s) nodes; for y in [y_m, y_{m+1}) it starts at
  clamp(m - (W/2 - 1), 0, NY_s - W).  A target node within 1e-14 of a source node copies it (a unit row).
* U(y) is interpolated with the same table.

States are global arrays in the one-rank ``get_state`` layout ``(NY, nkx, nkz)``, kx in the compact
order 0 .. Kx, -Kx .. -1, true Fourier coefficients.
"""
from __future__ import annotations

import math

import numpy as np

SNAP = 1e-14


def tanh_grid(N: int, stretch: float = 2.0) -> np.ndarray:
    """y_j = tanh(s (j dy - 1)) / tanh(s), the solver's wall-normal grid (libm tanh per node)."""
    dy = 2.0 / (N - 1)
    y = np.array([math.tanh(stretch * (j * dy - 1.0)) for j in range(N)]) / math.tanh(stretch)
    y[0], y[-1] = -1.0, 1.0
    return y


def interp_table(ys, yd, width: int = 6):
    """(j0[NY_d], w[NY_d, W]): target node j is sum_m w[j, m] f[j0[j] + m] of a source line f."""
    ys, yd = np.asarray(ys, float), np.asarray(yd, float)
    ns, W = len(ys), min(int(width), len(ys))
    j0 = np.zeros(len(yd), dtype=np.int64)
    w = np.zeros((len(yd), W))
    for j, y in enumerate(yd):
        m = int(np.searchsorted(ys, y, side="right")) - 1      # ys[m] <= y < ys[m + 1]
        m = min(max(m, 0), ns - 2)
        s = min(max(m - (W // 2 - 1), 0), ns - W)
        j0[j] = s
        nodes = ys[s:s + W]
        near = np.flatnonzero(np.abs(nodes - y) <= SNAP)
        if near.size:
            w[j, near[-1]] = 1.0
            continue
        for a in range(W):
            others = np.delete(nodes, a)
            w[j, a] = np.prod(y - others) / np.prod(nodes[a] - others)
    return j0, w


def apply_table(j0, w, f):
    """Interpolate along axis 0 of f (NY_s, ...) -> (NY_d, ...)."""
    f = np.asarray(f)
    out = np.zeros((len(j0),) + f.shape[1:], dtype=np.result_type(f.dtype, float))
    for j in range(len(j0)):
        unit = np.flatnonzero(w[j] == 1.0)
        if unit.size == 1 and np.count_nonzero(w[j]) == 1:
            out[j] = f[j0[j] + unit[0]]
            continue
        for m in range(w.shape[1]):
            out[j] += w[j, m] * f[j0[j] + m]
    return out


def mode_map(NX_s, NZ_s, NX_d, NZ_d):
    """(src[nkx_d], nkz_take): compact source kx index of every compact target kx index or -1, and the
    number of leading kz columns taken."""
    Ks, Kd = NX_s // 3, NX_d // 3
    nks, nkd = 2 * Ks + 1, 2 * Kd + 1
    src = np.full(nkd, -1, dtype=np.int64)
    for i in range(nkd):
        k = i if i <= Kd else i - nkd
        if abs(k) <= Ks:
            src[i] = k if k >= 0 else nks + k
    return src, min((2 * NZ_s - 2) // 3, (2 * NZ_d - 2) // 3) + 1


def plane_map(NX_s, NX_d):
    """FFT position in an NX_s-point array of every compact target kx index, or -1 (the file's planes)."""
    src, _ = mode_map(NX_s, 5, NX_d, 5)
    Ks = NX_s // 3
    return np.where(src < 0, -1, np.where(src <= Ks, src, NX_s - (2 * Ks + 1 - src)))


def regrid_state(phi, om, U, src, dst, width: int = 6):
    """(phi, om, U) on ``src = (NX, NY, NZ, stretch)`` -> the same on ``dst``."""
    NXs, NYs, NZs, ss = src
    NXd, NYd, NZd, sd = dst
    phi, om = np.asarray(phi, complex), np.asarray(om, complex)
    nks, nkzs = 2 * (NXs // 3) + 1, (2 * NZs - 2) // 3 + 1
    if phi.shape != (NYs, nks, nkzs) or om.shape != phi.shape:
        raise ValueError(f"source arrays must have shape {(NYs, nks, nkzs)}")
    j0, w = interp_table(tanh_grid(NYs, ss), tanh_grid(NYd, sd), width)
    kmap, ntake = mode_map(NXs, NZs, NXd, NZd)
    nkd, nkzd = 2 * (NXd // 3) + 1, (2 * NZd - 2) // 3 + 1
    out = []
    for f in (phi, om):
        g = np.zeros((NYd, nkd, nkzd), complex)
        have = kmap >= 0
        g[:, have, :ntake] = apply_table(j0, w, f[:, kmap[have], :ntake])
        out.append(g)
    return out[0], out[1], apply_table(j0, w, np.asarray(U, float))
