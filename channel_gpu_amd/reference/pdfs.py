"""NumPy reference of the per-plane histograms, the joint (u, v) histogram and the quadrant sums
(``Solver.plane_histograms``; the binning rule is the one of ``ZRealArgs::hist`` in kernels.hpp).

For a sample x, widened to double, of a field with centre c and half-width h at its plane:

  scale = nb / (2 h),   i = floor((x - c) * scale + nb / 2)    (product and sum rounded separately)
  bin   = 0 (underflow, i < 0 or x not a number) | nb + 1 (overflow, i >= nb) | i + 1

The joint histogram of (u, v) takes its index per axis from the 1-D bin, 0 | nj + 1 | i // (nb // nj) + 1,
so its marginals are the 1-D histograms re-binned.  The quadrants of u' = u - U and v are Q1 (u' >= 0,
v >= 0), Q2 (-, +), Q3 (-, -), Q4 (+, -).
"""
from __future__ import annotations

import numpy as np

HIST_NAMES = ("u", "v", "w", "wx", "wy", "wz")
# fields that change sign under the reflection y -> -y of the channel
ODD_FIELDS = ("v", "wx", "wz")


def bin_index(x, centre, scale, nb: int) -> np.ndarray:
    """1-D bin (0 .. nb + 1) of every sample of x."""
    f = np.floor((np.asarray(x, np.float64) - centre) * scale + nb / 2)
    inside = np.where(f >= nb, nb + 1, f + 1)
    return np.where(f >= 0, inside, 0).astype(np.int64)  # (not a number: bin 0)


def joint_index(b, nb: int, nj: int) -> np.ndarray:
    """Joint-histogram index per axis (0 .. nj + 1) of the 1-D bins b."""
    b = np.asarray(b, np.int64)
    return np.where(b == 0, 0, np.where(b == nb + 1, nj + 1, (b - 1) // (nb // nj) + 1))


def rebin(hist, nb: int, nj: int) -> np.ndarray:
    """A 1-D histogram [..., nb + 2] on the nj + 2 bins of a joint-histogram axis."""
    hist = np.asarray(hist)
    inner = hist[..., 1:-1].reshape(hist.shape[:-1] + (nj, nb // nj)).sum(-1)
    return np.concatenate([hist[..., :1], inner, hist[..., -1:]], -1)


def quadrant(du, v) -> np.ndarray:
    """0 .. 3 for Q1 .. Q4."""
    du, v = np.asarray(du), np.asarray(v)
    return np.where(du >= 0, np.where(v >= 0, 0, 3), np.where(v >= 0, 1, 2))


def histograms(phys, centre, halfwidth, nb: int, nj: int, U=None) -> dict:
    """phys: the fields u, v, w (and wx, wy, wz) as arrays (np, NX, Nzp), a sequence in that order or a
    dict by name; centre, halfwidth: (nhf, np).  U (np,): the mean that defines u' of the quadrant
    sums (default: the centre of u).  Returns hist (nhf, np, nb + 2) and joint (np, nj + 2, nj + 2),
    uint64, and quad (8, np): the plane means of u'v over Q1 .. Q4, then the quadrants' sample fractions."""
    if isinstance(phys, dict):
        phys = [phys[k] for k in HIST_NAMES if k in phys]
    phys = [np.asarray(a, np.float64) for a in phys]
    nhf, npl = len(phys), phys[0].shape[0]
    if nb < 2 or nb % 2 or nj < 1 or nb % nj:
        raise ValueError("nb must be even and a multiple of nj")
    centre = np.asarray(centre, np.float64).reshape(nhf, npl)
    halfwidth = np.asarray(halfwidth, np.float64).reshape(nhf, npl)
    U = centre[0] if U is None else np.asarray(U, np.float64).reshape(npl)
    hist = np.zeros((nhf, npl, nb + 2), np.uint64)
    joint = np.zeros((npl, nj + 2, nj + 2), np.uint64)
    quad = np.zeros((8, npl))
    for i in range(npl):
        b = [bin_index(phys[f][i], centre[f, i], nb / (2.0 * halfwidth[f, i]), nb) for f in range(nhf)]
        for f in range(nhf):
            hist[f, i] = np.bincount(b[f].ravel(), minlength=nb + 2)
        ju, jv = joint_index(b[0], nb, nj), joint_index(b[1], nb, nj)
        joint[i] = np.bincount((ju * (nj + 2) + jv).ravel(), minlength=(nj + 2) ** 2).reshape(nj + 2, nj + 2)
        du, v = phys[0][i] - U[i], phys[1][i]
        q = quadrant(du, v)
        for k in range(4):
            quad[k, i] = np.sum(np.where(q == k, du * v, 0.0)) / du.size
            quad[4 + k, i] = np.count_nonzero(q == k) / du.size
    return {"hist": hist, "joint": joint, "quad": quad}


def near_edge_count(x, centre, scale, nb: int, delta: float) -> int:
    """Samples of x within delta of an edge of the nb bins (the edges centre + (k - nb / 2) / scale,
    k = 0 .. nb): a sample perturbed by less than delta can change its bin only if it is one of them,
    and then by one bin."""
    t = (np.asarray(x, np.float64) - centre) * scale + nb / 2
    k = np.clip(np.rint(t), 0, nb)
    return int(np.count_nonzero(np.abs(t - k) <= delta * scale))


def near_axis_count(du, v, delta_u: float, delta_v: float) -> int:
    """Samples within delta of either axis of the quadrant split."""
    return int(np.count_nonzero((np.abs(np.asarray(du)) <= delta_u) | (np.abs(np.asarray(v)) <= delta_v)))


def moves(got, ref) -> int:
    """Distance between two 1-D histograms in adjacent-bin moves: sum_k |cum_got(k) - cum_ref(k)|."""
    d = np.cumsum(np.asarray(got, np.int64) - np.asarray(ref, np.int64), -1)
    return int(np.abs(d).sum())
