"""NumPy reference of the pressure on top of the oracle.

The solver advances du/dt = H - grad Pi + nu lap u with H = u x omega and Pi = p + |u|^2 / 2.  Per line
with k2 = al^2 + be^2 > 0, with the project's operators (compact D2 as M^-1 K, compact D1):

  interior rows   (K - k2 M) Pi = M S,   S = i al Hx + i be Hz + D1 Hy
  wall rows       (D1 Pi)(+-1) = Hy(+-1) + nu phi(+-1)

(the v-momentum equation at the wall, where v = 0 and D2 v = phi + k2 v = phi).  Solved like K-SPEC's
influence problem: Pi = Pi_p + c1 g1 + c2 g2 with Pi_p, g1, g2 from the Dirichlet matrix ``helm_matrix``
(right-hand sides M S, e_0, e_N) and c1, c2 from the 2 x 2 system of the first and last rows of the dense
D1.  The mean line (k2 = 0) is zero: only the fluctuating pressure is defined.

In physical space the fluctuating static pressure is p' = r - <r>_plane with
r = Pi' - U u' - (u'^2 + v^2 + w^2) / 2, u' = u - U(y); the plane-constant U^2 / 2 is dropped before r is
formed.
"""
from __future__ import annotations

import copy

import numpy as np

from .oracle import OracleSolver, _bsolve, helm_matrix, spec_to_phys_full

PRESSURE_ROWS = ("pp", "pu", "pv", "pw")


def rotational_hat(o: OracleSolver) -> np.ndarray:
    """H = u x omega of the prepared fields as [3, NY, lines]; ``o`` is left untouched."""
    if o.fields is None:
        o.prepare()
    c = copy.copy(o)
    c.transforms(compute_dt=False)
    return np.stack([c.lines(h) for h in c.H])


def pressure_hat(o: OracleSolver) -> np.ndarray:
    """Pi [NY, lines] of a prepared ``OracleSolver`` (one rank)."""
    ops, k2, al, be = o.ops, o.k2, o.al, o.be
    Hx, Hy, Hz = rotational_hat(o)
    phi = o.lines(o.phi)
    N, L = ops.N, k2.size
    S = 1j * al * Hx + 1j * be * Hz + ops.D1 @ Hy
    A = helm_matrix(ops, k2)
    e0 = np.zeros((N, L))
    e0[0] = 1.0
    eN = np.zeros((N, L))
    eN[-1] = 1.0
    Pp, g1, g2 = _bsolve(A, ops.M @ S), _bsolve(A, e0), _bsolve(A, eN)
    d0, dN = ops.D1[0], ops.D1[-1]
    b0 = Hy[0] + o.nu * phi[0] - d0 @ Pp
    bN = Hy[-1] + o.nu * phi[-1] - dN @ Pp
    a00, a01, a10, a11 = d0 @ g1, d0 @ g2, dN @ g1, dN @ g2
    det = a00 * a11 - a01 * a10
    c1 = (b0 * a11 - a01 * bN) / det
    c2 = (a00 * bN - a10 * b0) / det
    Pi = Pp + c1 * g1 + c2 * g2
    Pi[:, k2 == 0] = 0
    return Pi


def _physical(o: OracleSolver, Pi: np.ndarray):
    """(r, u', v, w) as [NY, NX, Nzp]."""
    sh = o.phi.shape
    P = np.array(Pi, complex).reshape(sh)
    if o.mean_line is not None:
        P[:, 0, 0] = 0
    Pp = spec_to_phys_full(P, o.plan)
    u, v, w = spec_to_phys_full(o.fields[:3], o.plan)
    U = np.asarray(o.U, float)[:, None, None]
    u = u - U
    return Pp - U * u - 0.5 * (u * u + v * v + w * w), u, v, w


def pressure_physical(o: OracleSolver, Pi: np.ndarray) -> np.ndarray:
    """p' [NY, NX, Nzp]: the fluctuating static pressure."""
    r = _physical(o, Pi)[0]
    return r - r.mean(axis=(1, 2), keepdims=True)


def pressure_moments(o: OracleSolver, Pi: np.ndarray) -> np.ndarray:
    """[4, NY] plane means <p'p'>, <p'u'>, <p'v>, <p'w> (``PRESSURE_ROWS``)."""
    r, u, v, w = _physical(o, Pi)
    p = r - r.mean(axis=(1, 2), keepdims=True)
    return np.stack([(p * q).mean(axis=(1, 2)) for q in (p, u, v, w)])


PSTRAIN_ROWS = ("ps_uu", "ps_vv", "ps_ww", "ps_uv", "pu", "pv", "pp_band")


def static_pressure_hat(o: OracleSolver, Pi: np.ndarray) -> np.ndarray:
    """p-hat' [NY, nkx, nkz]: the fluctuating static pressure back in spectral space, truncated to the
    retained modes, the mean line zero."""
    from .oracle import phys_to_spec_full

    p_hat = phys_to_spec_full(pressure_physical(o, Pi), o.plan)
    if o.mean_line is not None:
        p_hat[:, 0, 0] = 0
    return p_hat


def pressure_strain(o: OracleSolver, p_hat: np.ndarray) -> np.ndarray:
    """[7, NY] Parseval plane sums of p-hat' with the strain factors (``PSTRAIN_ROWS``; the weights and
    the wall-normal derivatives of ``budgets``): ps_uu = 2 <p' du'/dx>, ps_vv = 2 <p' dv/dy>,
    ps_ww = 2 <p' dw/dz>, ps_uv = <p' (du'/dy + dv/dx)>, <p'u'>, <p'v> and the retained-band part of
    <p'p'>.  The strain factors are band-limited to the retained modes, so the truncation of p' loses
    nothing in rows 0 to 5."""
    from .budgets import plane_weights, wall_normal_derivatives

    p = np.asarray(p_hat, complex).reshape(o.ops.N, -1)
    u, v, w = (o.lines(f) for f in o.fields[:3])
    du, dv, _ = wall_normal_derivatives(o)
    al, be = o.al, o.be
    dot = lambda a, b: a.real * b.real + a.imag * b.imag  # noqa: E731
    rows = [2.0 * dot(p, 1j * al * u), 2.0 * dot(p, dv), 2.0 * dot(p, 1j * be * w), dot(p, du + 1j * al * v),
            dot(p, u), dot(p, v), dot(p, p)]
    wgt = plane_weights(o)
    keep = wgt > 0
    return np.stack([r[:, keep] @ wgt[keep] for r in rows])


def momentum_residual(o: OracleSolver, Pi: np.ndarray, o_after: OracleSolver, dt: float):
    """(q1 - q0) / dt - (H - grad Pi + nu (D2 - k2) q0) for q = u, v, w as three [NY, lines] arrays:
    q0 the prepared fields of ``o``, q1 those of ``o_after`` (``o`` advanced over ``dt``).  Zeros for
    ``Pi`` leave the pressure gradient out."""
    ops, k2, al, be = o.ops, o.k2, o.al, o.be
    H = rotational_hat(o)
    Pi = np.asarray(Pi).reshape(ops.N, -1)
    grad = (1j * al * Pi, ops.D1 @ Pi, 1j * be * Pi)
    out = []
    for c in range(3):
        q0, q1 = o.lines(o.fields[c]), o_after.lines(o_after.fields[c])
        out.append((q1 - q0) / dt - (H[c] - grad[c] + o.nu * (ops.D2 @ q0 - k2 * q0)))
    return tuple(out)
