"""Velocity-gradient statistics on the CPU: the reference formulas (reference/budgets.py) against
physical-space gradients and against the oracle's own energy balance, and the budget profiles of
TurbulenceStatistics against direct NumPy expressions."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import BUDGET_STRESSES, BUDGET_TERMS, TurbulenceStatistics
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora


def _fluct(o, f):
    """[NY, nkx, nkz] field with the mean line removed."""
    g = np.array(f)
    g[:, 0, 0] = 0
    return g


def test_parseval_rows_match_plane_means():
    """Every row of gradient_sums equals the plane mean of the physical-space expression, the
    gradients being (i al f, D f, i be f) with the solver's own D.  Measured 1.4e-15 of each row's
    maximum; bound 1e-12."""
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    got = bud.gradient_sums(o)
    assert got.shape == (7, 33)
    sh = o.phi.shape
    al, be = o.al.reshape(sh[1:]), o.be.reshape(sh[1:])
    u, v, w, wx, wy, wz = (_fluct(o, f) for f in o.fields)
    du, dv, dw = (_fluct(o, d.reshape(sh)) for d in bud.wall_normal_derivatives(o))
    phys = lambda f: ora.spec_to_phys_full(f, o.plan)  # noqa: E731
    grad = {n: [phys(1j * al * f), phys(d), phys(1j * be * f)] for n, f, d in (("u", u, du), ("v", v, dv), ("w", w, dw))}
    gdot = lambda a, b: sum((x * y).mean(axis=(1, 2)) for x, y in zip(grad[a], grad[b]))  # noqa: E731
    ref = np.stack([(phys(wx) ** 2).mean(axis=(1, 2)), (phys(wy) ** 2).mean(axis=(1, 2)), (phys(wz) ** 2).mean(axis=(1, 2)),
                    gdot("u", "u"), gdot("v", "v"), gdot("w", "w"), gdot("u", "v")])
    for r in range(7):
        err = np.abs(got[r] - ref[r]).max() / np.abs(ref[r]).max()
        print(f"row {bud.GRADIENT_ROWS[r]}: rel. error {err:.2e}")
        assert err < 1e-12


def test_energy_balance():
    """dK/dt = int (P_k - eps_k) dy for the oracle's own step (the transport and diffusion terms
    integrate to zero between the walls): pins nu and the factor 2 independently of the formulas.
    Central difference over two steps of dt = 1e-3 about the middle state; measured 4.4e-4 of
    int eps (production is 45 % of eps there); a wrong factor 2 or a missing nu gives >= 0.4."""
    dt = 1e-3
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=100.0, dt_fixed=dt)
    phi, om = bud.smooth_state(o.plan, o.ops, seed=3, amp=0.05, kscale=4)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    K = lambda: 0.5 * o.ops.trap @ o.plane_stats()[:3].sum(axis=0)  # noqa: E731
    K0 = K()
    o.step()
    st, g = o.plane_stats(), bud.gradient_sums(o)
    prod = o.ops.trap @ (-st[3] * (o.ops.D1 @ o.U))
    eps = o.ops.trap @ (o.nu * (g[3] + g[4] + g[5]))
    o.step()
    K2 = K()
    dK = (K2 - K0) / (2 * dt)
    err = abs(dK - (prod - eps)) / eps
    print(f"dK/dt {dK:.6e}  P {prod:.6e}  eps {eps:.6e}  P/eps {prod / eps:.3f}  |difference| / eps {err:.2e}")
    assert prod > 0.2 * eps  # (production is exercised)
    assert err < 2e-3


@functools.lru_cache(maxsize=None)
def _synthetic(n=33):
    """One asymmetric synthetic sample (no parity in y): U, stats [4, n], grad [7, n], triple [3, n], vvv."""
    rng = np.random.default_rng(5)
    y = ora.ygrid(n)
    smooth = lambda: (1 - y ** 2) * (rng.uniform(-1, 1) + rng.uniform(-1, 1) * y + rng.uniform(-1, 1) * y ** 2 +  # noqa: E731
                                      rng.uniform(-1, 1) * y ** 3)
    U = 1.35 * (1 - y ** 2) * (1 + 0.1 * y)
    st = np.stack([smooth() ** 2 + 0.1 * (1 - y ** 2), smooth() ** 2, smooth() ** 2, smooth()])
    grad = np.stack([np.abs(smooth()) + 0.3 + 0.1 * y for _ in range(6)] + [smooth()])
    triple = np.stack([smooth() for _ in range(3)])
    return y, U, st, grad, triple, smooth()


def test_statistics_budget_terms():
    y, U, st, grad, triple, vvv = _synthetic()
    n, nu = y.size, 1.0 / 180.0
    ops = ora.build_ops(n)
    S = TurbulenceStatistics(y, nu)
    ut_lo, ut_hi = 0.06, 0.07
    S.add(U, st.ravel(), ut_lo, ut_hi, 0.0)
    S.add_budgets(grad, triple, vvv)
    b = S.budgets()
    uu, vv, ww, uv = st
    dU = ops.D1 @ U
    ref = {
        "prod_k": -uv * dU, "prod_uu": -2 * uv * dU, "prod_vv": 0 * U, "prod_ww": 0 * U, "prod_uv": -vv * dU,
        "eps_k": nu * (grad[3] + grad[4] + grad[5]), "eps_uu": 2 * nu * grad[3], "eps_vv": 2 * nu * grad[4],
        "eps_ww": 2 * nu * grad[5], "eps_uv": 2 * nu * grad[6],
        "visc_k": nu * ops.D2 @ (0.5 * (uu + vv + ww)), "visc_uu": nu * ops.D2 @ uu, "visc_vv": nu * ops.D2 @ vv,
        "visc_ww": nu * ops.D2 @ ww, "visc_uv": nu * ops.D2 @ uv,
        "turb_k": -ops.D1 @ (0.5 * (triple[0] + vvv + triple[1])), "turb_uu": -ops.D1 @ triple[0],
        "turb_vv": -ops.D1 @ vvv, "turb_ww": -ops.D1 @ triple[1], "turb_uv": -ops.D1 @ triple[2],
    }
    for s in BUDGET_STRESSES:
        ref["resid_" + s] = -(ref["prod_" + s] - ref["eps_" + s] + ref["visc_" + s] + ref["turb_" + s])
    assert sorted(b) == sorted(f"{t}_{s}" for s in BUDGET_STRESSES for t in BUDGET_TERMS)
    for k, r in ref.items():
        scale = max(np.abs(r).max(), 1e-300)
        assert np.abs(b[k] - r).max() <= 1e-12 * scale, k
    assert np.array_equal(b["resid_k"], -(b["prod_k"] - b["eps_k"] + b["visc_k"] + b["turb_k"]))

    # folded wall-unit profiles: (a[lo] + s a[hi]) / 2 with s = -1 for every term of the uv budget
    p = S.profiles()
    ut = np.sqrt(0.5 * (ut_lo ** 2 + ut_hi ** 2))
    h = (n + 1) // 2
    lo, hi = np.arange(h), n - 1 - np.arange(h)
    for k, r in ref.items():
        sgn = -1.0 if k.endswith("_uv") else 1.0
        want = 0.5 * (r[lo] + sgn * r[hi]) * nu / ut ** 4
        assert p[k].shape == (h,)
        assert np.abs(p[k] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), k
        # (the asymmetric input tells the two parities apart)
        other = 0.5 * (r[lo] - sgn * r[hi]) * nu / ut ** 4
        if np.abs(r).max() > 0:
            assert np.abs(p[k] - other).max() > 1e-6 * np.abs(want).max(), k
    for q, name in enumerate(("wx_rms", "wy_rms", "wz_rms")):
        want = np.sqrt(0.5 * (grad[q][lo] + grad[q][hi])) * nu / ut ** 2
        assert np.abs(p[name] - want).max() <= 1e-12 * want.max()
    assert np.array_equal(p["prod_vv"], np.zeros(h))


def test_statistics_write_appends_budget_columns(tmp_path):
    y, U, st, grad, triple, vvv = _synthetic()
    S = TurbulenceStatistics(y, 1.0 / 180.0)
    S.add(U, st.ravel(), 0.06, 0.07, 0.0)
    S.write(str(tmp_path / "a.dat"))
    base = np.loadtxt(tmp_path / "a.dat")
    S.add_budgets(grad, triple, vvv)
    S.write(str(tmp_path / "b.dat"))
    full = np.loadtxt(tmp_path / "b.dat")
    assert full.shape == (base.shape[0], base.shape[1] + 3 + 25)
    names = (tmp_path / "b.dat").read_text().splitlines()[1].split()[1:]
    assert names[-25:] == [f"{t}_{s}" for s in BUDGET_STRESSES for t in BUDGET_TERMS] and names[-28] == "wx_rms"
    p = S.profiles()
    assert np.allclose(full[:, names.index("resid_k")], p["resid_k"], rtol=1e-6, atol=1e-12)


def test_config_key_budget_every():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    assert C.Config().budget_every == 0
    c = default_config(NX=32, NY=33, NZ=17, budget_every=6)
    assert C.Config.from_string(c.to_string()).budget_every == 6
    assert C.Config.from_string("NX = 32; NY = 33; NZ = 17; budget_every = 3;").budget_every == 3
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, budget_every=-1)


def test_budgets_need_samples():
    S = TurbulenceStatistics(ora.ygrid(17), 0.01)
    with pytest.raises(ValueError):
        S.budgets()
