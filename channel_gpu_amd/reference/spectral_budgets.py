"""NumPy reference of the spectral Reynolds-stress budgets at every plane (``Solver.spectral_budgets``;
csrc/include/channel/kernels.hpp SBudgetArgs) on top of the oracle.

The solver advances du/dt = H - grad Pi + nu lap u with H = u x omega and Pi = p + |u|^2 / 2.  With
u = U(y) e_x + u' and omega = -U' e_z + omega', for every retained mode off the mean line

  H = H_lin + H',   H_lin = (-U' v, U' u - U omega_z, U omega_y),   H' = (u' x omega')^
  G = Pi - U u = (p' + |u'|^2 / 2)^

(the U u' parts of H and of grad Pi cancel).  With a.b = Re(a b*), E_ab = a.b per mode and the solver's
own wall-normal derivatives D (``budgets.wall_normal_derivatives``):

  dt E_uu = -2 U' (u.v) + 2 n_uu + gs_uu            + nu (D2 E_uu - 2 g_uu)
  dt E_vv =               2 n_vv + gs_vv - 2 D1(gv) + nu (D2 E_vv - 2 g_vv)
  dt E_ww =               2 n_ww + gs_ww            + nu (D2 E_ww - 2 g_ww)
  dt E_uv = -U' E_vv   +    n_uv + gs_uv -   D1(gu) + nu (D2 E_uv - 2 g_uv)

  n_uu = u.H'x, n_vv = v.H'y, n_ww = w.H'z, n_uv = u.H'y + v.H'x
  g_ab = k2 a.b + Da.Db                      (the summands of ``budgets.gradient_sums`` rows 3..6)
  gs_uu = 2 G.(i al u), gs_vv = 2 G.Dv, gs_ww = 2 G.(i be w), gs_uv = G.(Du + i al v);  gu = G.u, gv = G.v
  ps_*, pu, pv: the same six with p' for G   (the summands of ``pressure.pressure_strain`` rows 0..5)

gs_uu + gs_vv + gs_ww = 0 and ps_uu + ps_vv + ps_ww = 0 per mode (continuity).  The conventional split is
arithmetic on these rows: turbulent transport plus inter-scale transfer of uu is 2 n_uu + gs_uu - ps_uu,
pressure diffusion of vv is -2 D1(pv), production comes from the uv and vv rows of the plane spectra.

Binning as ``spectra.plane_spectra``: weight 1 for kz = 0 and 2 for kz > 0, the mean line excluded, +kx
and -kx in the bin |kx|.
"""
from __future__ import annotations

import numpy as np

from . import pressure as prs
from .budgets import plane_weights, wall_normal_derivatives
from .oracle import OracleSolver

SBUDGET_ROWS = ("n_uu", "n_vv", "n_ww", "n_uv", "g_uu", "g_vv", "g_ww", "g_uv", "gs_uu", "gs_vv", "gs_ww", "gs_uv",
                "gu", "gv", "ps_uu", "ps_vv", "ps_ww", "ps_uv", "pu", "pv")
ROW = {name: i for i, name in enumerate(SBUDGET_ROWS)}
STRESSES = ("uu", "vv", "ww", "uv")


def _dot(a, b):
    return a.real * b.real + a.imag * b.imag


def mode_rows(o: OracleSolver, H=None, Pi=None, p_hat=None) -> np.ndarray:
    """The 20 rows per mode, unweighted, as [20, NY, lines], of a prepared ``OracleSolver`` (one rank).
    ``H`` [3, NY, lines], ``Pi`` and ``p_hat`` [NY, lines] default to ``pressure.rotational_hat``,
    ``pressure_hat`` and ``static_pressure_hat``.  The mean line is not meaningful."""
    if o.fields is None:
        o.prepare()
    N = o.ops.N
    u, v, w, _, wy, wz = (o.lines(f) for f in o.fields)
    du, dv, dw = wall_normal_derivatives(o)
    al, be, k2 = o.al, o.be, o.k2
    U = np.asarray(o.U, float)[:, None]
    dU = (o.ops.D1 @ np.asarray(o.U, float))[:, None]
    H = prs.rotational_hat(o) if H is None else np.asarray(H, complex).reshape(3, N, -1)
    Pi = prs.pressure_hat(o) if Pi is None else np.asarray(Pi, complex).reshape(N, -1)
    p = prs.static_pressure_hat(o, Pi) if p_hat is None else p_hat
    p = np.asarray(p, complex).reshape(N, -1)
    hx = H[0] + dU * v
    hy = H[1] - (dU * u - U * wz)
    hz = H[2] - U * wy
    G = Pi - U * u
    sxx, syy, szz, sxy = 1j * al * u, dv, 1j * be * w, du + 1j * al * v
    rows = [_dot(u, hx), _dot(v, hy), _dot(w, hz), _dot(u, hy) + _dot(v, hx),
            k2 * _dot(u, u) + _dot(du, du), k2 * _dot(v, v) + _dot(dv, dv), k2 * _dot(w, w) + _dot(dw, dw),
            k2 * _dot(u, v) + _dot(du, dv)]
    for q in (G, p):
        part = [2.0 * _dot(q, sxx), 2.0 * _dot(q, syy), 2.0 * _dot(q, szz), _dot(q, sxy), _dot(q, u), _dot(q, v)]
        rows += part
    return np.stack(rows)


def bin_rows(o: OracleSolver, rows: np.ndarray):
    """Per-mode rows [R, NY, lines] -> (ekx [R, NY, Kx + 1], ekz [R, NY, nkz]), weighted."""
    p = o.plan
    wgt = plane_weights(o)
    prod = np.where(wgt > 0, rows, 0.0) * wgt
    prod = prod.reshape(rows.shape[0], p.NY, p.nkx_loc, p.nkz_loc)
    ekx = np.zeros((rows.shape[0], p.NY, p.Kx + 1))
    ekz = np.zeros((rows.shape[0], p.NY, p.nkz))
    akx = np.abs(p.kx_of(p.kx0 + np.arange(p.nkx_loc)))
    np.add.at(ekx, (slice(None), slice(None), akx), prod.sum(axis=3))
    ekz[:, :, p.kz0:p.kz0 + p.nkz_loc] = prod.sum(axis=2)
    return ekx, ekz


def spectral_budgets(o: OracleSolver, H=None, Pi=None, p_hat=None) -> dict:
    """``{"rows", "ekx" [20, NY, Kx + 1], "ekz" [20, NY, nkz], "U", "dU"}`` of a prepared ``OracleSolver``."""
    ekx, ekz = bin_rows(o, mode_rows(o, H, Pi, p_hat))
    U = np.array(o.U, float)
    return {"rows": SBUDGET_ROWS, "ekx": ekx, "ekz": ekz, "U": U, "dU": o.ops.D1 @ U}


def stress_rows(o: OracleSolver) -> np.ndarray:
    """E_uu, E_vv, E_ww, E_uv per mode, [4, NY, lines]."""
    u, v, w = (o.lines(f) for f in o.fields[:3])
    return np.stack([_dot(u, u), _dot(v, v), _dot(w, w), _dot(u, v)])


def budget_terms(ops, nu, U, rows, E) -> dict:
    """The terms of the four budgets from the rows: ``rows`` [20, NY, ...] and the stresses ``E``
    [4, NY, ...] (uu, vv, ww, uv) over any trailing axes (modes or bins).  Returns ``{stress: {term: array}}``
    with the terms production, nonlinear (turbulent transport plus inter-scale transfer), pressure_strain,
    pressure_diffusion, viscous_diffusion, dissipation; their sum is dt E."""
    r = {n: rows[i] for n, i in ROW.items()}
    sh = (-1,) + (1,) * (rows.ndim - 2)
    dU = (ops.D1 @ np.asarray(U, float)).reshape(sh)
    d1 = lambda a: np.tensordot(ops.D1, a, axes=(1, 0))  # noqa: E731
    d2 = lambda a: np.tensordot(ops.D2, a, axes=(1, 0))  # noqa: E731
    zero = np.zeros_like(E[0])
    prod = {"uu": -2.0 * dU * E[3], "vv": zero, "ww": zero, "uv": -dU * E[1]}
    fac = {"uu": 2.0, "vv": 2.0, "ww": 2.0, "uv": 1.0}
    # D1 of (G - p) q completes the nonlinear term: gs - ps - f D1((G - p).q) is the part of |u'|^2 / 2
    pd = {"uu": zero, "vv": -2.0 * d1(r["pv"]), "ww": zero, "uv": -d1(r["pu"])}
    gd = {"uu": zero, "vv": -2.0 * d1(r["gv"]), "ww": zero, "uv": -d1(r["gu"])}
    out = {}
    for i, s in enumerate(STRESSES):
        out[s] = {
            "production": prod[s],
            "nonlinear": fac[s] * r["n_" + s] + r["gs_" + s] - r["ps_" + s] + gd[s] - pd[s],
            "pressure_strain": r["ps_" + s],
            "pressure_diffusion": pd[s],
            "viscous_diffusion": nu * d2(E[i]),
            "dissipation": -2.0 * nu * r["g_" + s],
        }
    return out
