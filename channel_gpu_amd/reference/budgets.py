"""NumPy reference of the velocity-gradient statistics (vorticity r.m.s., dissipation, the triple
products of the turbulent transport) on top of the oracle.

Conventions (shared with the device kernels, csrc/include/channel/kernels.hpp GradSumArgs):
  * fluctuations exclude the mean line (kx = 0, kz = 0) completely;
  * plane mean of a product <a'b'>(y) = sum over the retained (kx, kz) of w(kz) Re(a conj b), w = 1 for
    kz = 0 and 2 for kz > 0 (the weight of ``OracleSolver.plane_stats``);
  * the wall-normal derivatives are the solver's own, the ones its vorticity is built from:
    D u = i al v - omega_z, D w = omega_x + i be v, D v = -i (al u + be w) -- not D1 applied to u.
"""
from __future__ import annotations

import math

import numpy as np

from .oracle import OraclePlan, OracleSolver, YOps

GRADIENT_ROWS = ("wxwx", "wywy", "wzwz", "guu", "gvv", "gww", "guv")
TRANSPORT_ROWS = ("uuv", "wwv", "uvv")


def plane_weights(o: OracleSolver) -> np.ndarray:
    """Per local line: 1 (kz = 0), 2 (kz > 0), 0 on the mean line."""
    p = o.plan
    wgt = np.where(np.tile(p.kz0 + np.arange(p.nkz_loc), p.nkx_loc) == 0, 1.0, 2.0)
    if o.mean_line is not None:
        wgt[o.mean_line] = 0.0
    return wgt


def wall_normal_derivatives(o: OracleSolver):
    """(D u, D v, D w) of the prepared fields as [NY, lines] (the mean line is not meaningful)."""
    u, v, w, wx, _, wz = (o.lines(f) for f in o.fields)
    al, be = o.al, o.be
    return 1j * al * v - wz, -1j * (al * u + be * w), wx + 1j * be * v


def gradient_sums(o: OracleSolver) -> np.ndarray:
    """[7, NY] raw plane sums (``GRADIENT_ROWS``; no nu, no factor 2) of a prepared ``OracleSolver``
    (this rank's lines; a distributed caller sums over the ranks)."""
    if o.fields is None:
        o.prepare()
    u, v, w, wx, wy, wz = (o.lines(f) for f in o.fields)
    du, dv, dw = wall_normal_derivatives(o)
    wgt, k2 = plane_weights(o), o.k2
    sq = lambda a: a.real ** 2 + a.imag ** 2  # noqa: E731
    dot = lambda a, b: a.real * b.real + a.imag * b.imag  # noqa: E731
    rows = [sq(wx), sq(wy), sq(wz), k2 * sq(u) + sq(du), k2 * sq(v) + sq(dv), k2 * sq(w) + sq(dw),
            k2 * dot(u, v) + dot(du, dv)]
    # (the weight is applied by selection: the mean line of u and omega_z holds U and -U', not a fluctuation)
    keep = wgt > 0
    return np.stack([r[:, keep] @ wgt[keep] for r in rows])


def transport_moments(phys6: np.ndarray, U: np.ndarray) -> np.ndarray:
    """[3, NY] plane means of u'u'v, w w v, u'v v (``TRANSPORT_ROWS``) of the physical fields
    [>= 3, NY, NX, Nzp] (u, v, w first), u' = u - U(y)."""
    u = phys6[0] - np.asarray(U, float)[:, None, None]
    v, w = phys6[1], phys6[2]
    return np.stack([(u * u * v).mean(axis=(1, 2)), (w * w * v).mean(axis=(1, 2)), (u * v * v).mean(axis=(1, 2))])


def smooth_state(plan: OraclePlan, ops: YOps, seed: int = 1, amp: float = 0.1, kscale: float = 32.0):
    """Like ``oracle.random_state`` but smooth in y: per mode v = amp e^(-k2/kscale) (1-y^2)^2 (c0 + c1 y
    + c2 y^2) and omega_y = amp e^(-k2/kscale) (1-y^2) (d0 + d1 y + d2 y^2) with complex coefficients
    uniform in [-1, 1], phi = D2 v - k2 v, Hermitian kz = 0."""
    rng = np.random.default_rng(seed)
    N, y = ops.N, ops.y
    gphi = np.zeros((N, plan.nkx, plan.nkz), complex)
    gom = np.zeros_like(gphi)
    pw = np.stack([np.ones(N), y, y * y])
    for i in range(plan.nkx):
        kx = int(plan.kx_of(i))
        if kx < 0:
            continue
        for kz in range(plan.nkz):
            if kx == 0 and kz == 0:
                continue
            al, be = plan.ax * kx, plan.az * kz
            k2 = al * al + be * be
            env = math.exp(-k2 / kscale)
            c = rng.uniform(-1, 1, 3) + 1j * rng.uniform(-1, 1, 3)
            d = rng.uniform(-1, 1, 3) + 1j * rng.uniform(-1, 1, 3)
            v = amp * env * (1 - y ** 2) ** 2 * (c @ pw)
            om = amp * env * (1 - y ** 2) * (d @ pw)
            phi = ops.D2 @ v - k2 * v
            gphi[:, i, kz], gom[:, i, kz] = phi, om
            if kz == 0 and kx > 0:
                j = plan.nkx - kx
                gphi[:, j, 0], gom[:, j, 0] = np.conj(phi), np.conj(om)
    return gphi, gom
