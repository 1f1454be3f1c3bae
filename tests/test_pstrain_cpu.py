"""Pressure strain on the CPU: the NumPy reference (reference/pressure.py static_pressure_hat,
pressure_strain) against physical-space plane means and in the oracle's own component energy balances,
the pressure-strain profiles of TurbulenceStatistics on synthetic sums, and the config key."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import PSTRAIN_ROWS, PSTRAIN_TERMS, TurbulenceStatistics
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs


@functools.lru_cache(maxsize=None)
def _case():
    """The state of tests/test_pressure_gpu.py at 32x33x17 (random_state seed 9, amp 0.3, Re 400,
    parabolic U): the oracle, Pi, p-hat' and the reference rows; computed once, read-only."""
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    Pi = prs.pressure_hat(o)
    ph = prs.static_pressure_hat(o, Pi)
    rows = prs.pressure_strain(o, ph)
    for a in (Pi, ph, rows):
        a.setflags(write=False)
    return o, Pi, ph, rows


def test_reference_rows_against_physical_space():
    """Rows 0 to 5 are the physical-space plane means of p' times the gradient (or velocity), the
    factors transformed with spec_to_phys_full: < 1e-12 of each row's maximum (measured <= 6e-16).  Row
    6 is the retained-band part of <p'p'>: 0 < pp_band <= <p'p'> on interior planes (measured ratio
    0.99988 to 1.0)."""
    o, Pi, ph, rows = _case()
    assert prs.PSTRAIN_ROWS == PSTRAIN_ROWS and rows.shape == (7, 33)
    assert ph.shape == o.phi.shape and np.array_equal(ph[:, 0, 0], np.zeros(33, complex))
    sh = o.phi.shape
    p = prs.pressure_physical(o, Pi)
    u, v, w = (o.lines(f) for f in o.fields[:3])
    du, dv, _ = bud.wall_normal_derivatives(o)
    al, be = o.al, o.be

    def phys(a):
        a = np.array(a, complex).reshape(sh)
        a[:, 0, 0] = 0  # (fluctuations: the mean line of u holds U)
        return ora.spec_to_phys_full(a, o.plan)

    want = [2 * p * phys(1j * al * u), 2 * p * phys(dv), 2 * p * phys(1j * be * w), p * phys(du + 1j * al * v),
            p * phys(u), p * phys(v)]
    for q, f in enumerate(want):
        m = f.mean(axis=(1, 2))
        err = np.abs(rows[q] - m).max() / np.abs(m).max()
        print(f"{PSTRAIN_ROWS[q]}: Parseval against the physical-space plane mean, rel. error {err:.2e} (tol 1e-12)")
        assert err < 1e-12, PSTRAIN_ROWS[q]
    pp = (p * p).mean(axis=(1, 2))
    ratio = rows[6][1:-1] / pp[1:-1]
    print(f"pp_band / <p'p'> on interior planes: {ratio.min():.6f} to {ratio.max():.6f}")
    assert (rows[6][1:-1] > 0).all() and (rows[6][1:-1] <= pp[1:-1]).all()


def test_reference_identities():
    """Rows pu and pv are rows 1 and 2 of pressure_moments (u', v are band-limited), and the trace
    ps_uu + ps_vv + ps_ww is zero by continuity: 1e-12 of the largest row."""
    o, Pi, ph, rows = _case()
    pm = prs.pressure_moments(o, Pi)
    for q, r in ((4, 1), (5, 2)):
        err = np.abs(rows[q] - pm[r]).max() / np.abs(pm[r]).max()
        print(f"{PSTRAIN_ROWS[q]} against pressure_moments row {r}: rel. error {err:.2e} (tol 1e-12)")
        assert err < 1e-12
    tr = np.abs(rows[0] + rows[1] + rows[2]).max() / np.abs(rows[:3]).max()
    print(f"|ps_uu + ps_vv + ps_ww| / max row: {tr:.2e} (tol 1e-12)")
    assert tr <= 1e-12


# |d/dt int <q q> dy - int (terms) dy| / int eps: about three times the measured 1.4e-3, 1.1e-2, 2.7e-5
# (the y-discretisation's error: 2.1e-4, 1.6e-3, 1.3e-5 at 16x129x9)
BALANCE_BOUNDS = (5e-3, 3e-2, 1e-3)


def test_component_energy_balance():
    """d/dt int <u'u'> dy = int (2 P_k - eps_uu + ps_uu) dy, d/dt int <vv> dy = int (-eps_vv + ps_vv) dy,
    d/dt int <ww> dy = int (-eps_ww + ps_ww) dy on the oracle's own step (transport and diffusion
    integrate to zero between the walls): pins the sign and the factor 2 of the pressure-strain rows
    independently of the formulas.  Central difference over two steps of dt = 1e-3 about the middle
    state.  Measured |difference| / int eps: uu 1.4e-3, vv 1.1e-2, ww 2.7e-5; with half the
    pressure-strain term 6e-2, 0.56, 0.115; without it 0.12, 1.1, 0.23."""
    dt = 1e-3
    o = ora.OracleSolver(NX=32, NY=65, NZ=17, Re=100.0, dt_fixed=dt)
    phi, om = bud.smooth_state(o.plan, o.ops, seed=3, amp=0.3, kscale=4)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    trap = o.ops.trap
    E = lambda: trap @ o.plane_stats()[:3].T  # noqa: E731
    E0 = E()
    o.step()
    st, g = o.plane_stats(), bud.gradient_sums(o)
    ps = prs.pressure_strain(o, prs.static_pressure_hat(o, prs.pressure_hat(o)))
    prod = np.array([trap @ (-2.0 * st[3] * (o.ops.D1 @ o.U)), 0.0, 0.0])
    eps = np.array([trap @ (2.0 * o.nu * g[3 + c]) for c in range(3)])
    pst = np.array([trap @ ps[c] for c in range(3)])
    o.step()
    dE = (E() - E0) / (2 * dt)
    for c, name in enumerate(("uu", "vv", "ww")):
        err = abs(dE[c] - (prod[c] - eps[c] + pst[c])) / eps[c]
        half = abs(dE[c] - (prod[c] - eps[c] + 0.5 * pst[c])) / eps[c]
        none = abs(dE[c] - (prod[c] - eps[c])) / eps[c]
        print(f"{name}: dE/dt {dE[c]:.6e} P {prod[c]:.6e} eps {eps[c]:.6e} ps {pst[c]:.6e}  |difference| / eps {err:.2e} "
              f"(bound {BALANCE_BOUNDS[c]:.0e}); half the term {half:.2e}, without {none:.2e}")
        assert err < BALANCE_BOUNDS[c], name
        assert half >= 10 * BALANCE_BOUNDS[c], name  # (the test cannot pass by slack)


@functools.lru_cache(maxsize=None)
def _synthetic(n=33):
    """One asymmetric synthetic sample (no parity in y)."""
    rng = np.random.default_rng(17)
    y = ora.ygrid(n)
    smooth = lambda: (1 - y ** 2) * (rng.uniform(-1, 1) + rng.uniform(-1, 1) * y + rng.uniform(-1, 1) * y ** 2 +  # noqa: E731
                                      rng.uniform(-1, 1) * y ** 3)
    U = 1.35 * (1 - y ** 2) * (1 + 0.1 * y)
    st = np.stack([smooth() ** 2 + 0.1 * (1 - y ** 2), smooth() ** 2, smooth() ** 2, smooth()])
    grad = np.stack([np.abs(smooth()) + 0.3 + 0.1 * y for _ in range(6)] + [smooth()])
    triple = np.stack([smooth() for _ in range(3)])
    pm = np.stack([smooth() ** 2 + 0.2 + 0.05 * y, smooth() + 0.1 * y, smooth(), smooth()])
    ps = np.stack([smooth() + 0.1 * y for _ in range(6)] + [smooth() ** 2])
    return y, U, st, grad, triple, smooth(), pm, ps


def test_statistics_pressure_strain_profiles():
    y, U, st, grad, triple, vvv, pm, ps = _synthetic()
    n, nu = y.size, 1.0 / 180.0
    S = TurbulenceStatistics(y, nu)
    with pytest.raises(ValueError):
        S.pressure_strain_terms()
    ut_lo, ut_hi = 0.06, 0.07
    S.add(U, st.ravel(), ut_lo, ut_hi, 0.0)
    assert "pstrain_uu" not in S.profiles()
    # two samples: the averages are formed first
    S.add_pressure_strain(0.5 * ps)
    S.add_pressure_strain(1.5 * ps)
    assert S.nps == 2 and len(PSTRAIN_ROWS) == 7
    t = S.pressure_strain_terms()
    assert sorted(t) == sorted(PSTRAIN_TERMS)
    for q, k in enumerate(PSTRAIN_TERMS):
        assert np.abs(t[k] - ps[q]).max() <= 1e-12 * np.abs(ps[q]).max(), k
    p = S.profiles()
    assert not [k for k in p if k.startswith("closure_")]  # (need the budgets and the pressure moments)
    ut = np.sqrt(0.5 * (ut_lo ** 2 + ut_hi ** 2))
    h = (n + 1) // 2
    lo, hi = np.arange(h), n - 1 - np.arange(h)
    fold = lambda a, s: 0.5 * (a[lo] + s * a[hi])  # noqa: E731
    for q, k in enumerate(PSTRAIN_TERMS):
        s = -1.0 if k == "pstrain_uv" else 1.0
        w, other = fold(ps[q], s) * nu / ut ** 4, fold(ps[q], -s) * nu / ut ** 4
        assert p[k].shape == (h,), k
        assert np.abs(p[k] - w).max() <= 1e-12 * np.abs(w).max(), k
        # (the asymmetric input tells the two parities apart)
        assert np.abs(p[k] - other).max() > 1e-6 * np.abs(w).max(), k
    # with the budgets alone, or the pressure moments alone: still no per-component closure
    S.add_budgets(grad, triple, vvv)
    assert "closure_uu" not in S.profiles()
    S.add_pressure(pm)
    q = S.profiles()
    assert np.array_equal(q["closure_uu"], q["resid_uu"] - q["pstrain_uu"])
    assert np.array_equal(q["closure_ww"], q["resid_ww"] - q["pstrain_ww"])
    assert np.array_equal(q["closure_vv"], q["resid_vv"] - q["pdiff_vv"] - q["pstrain_vv"])
    assert np.array_equal(q["closure_uv"], q["resid_uv"] - q["pdiff_uv"] - q["pstrain_uv"])
    # the existing keys keep their values
    S2 = TurbulenceStatistics(y, nu)
    S2.add(U, st.ravel(), ut_lo, ut_hi, 0.0)
    S2.add_budgets(grad, triple, vvv)
    S2.add_pressure(pm)
    q2 = S2.profiles()
    for k, a in q2.items():
        assert np.array_equal(a, q[k]), k
    new = list(PSTRAIN_TERMS) + ["closure_uu", "closure_vv", "closure_ww", "closure_uv"]
    assert sorted(set(q) - set(q2)) == sorted(new)


def test_statistics_write_appends_pressure_strain_columns(tmp_path):
    y, U, st, grad, triple, vvv, pm, ps = _synthetic()
    S = TurbulenceStatistics(y, 1.0 / 180.0)
    S.add(U, st.ravel(), 0.06, 0.07, 0.0)
    S.add_budgets(grad, triple, vvv)
    S.add_pressure(pm)
    S.write(str(tmp_path / "a.dat"))
    base = np.loadtxt(tmp_path / "a.dat")
    S.add_pressure_strain(ps)
    S.write(str(tmp_path / "b.dat"))
    full = np.loadtxt(tmp_path / "b.dat")
    assert full.shape == (base.shape[0], base.shape[1] + 8)
    names = (tmp_path / "b.dat").read_text().splitlines()[1].split()[1:]
    assert names[-8:] == list(PSTRAIN_TERMS) + ["closure_uu", "closure_vv", "closure_ww", "closure_uv"]
    assert np.allclose(full[:, names.index("closure_vv")], S.profiles()["closure_vv"], rtol=1e-6, atol=1e-12)


def test_config_key():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    assert C.Config().pstrain_every == 0
    c = default_config(NX=32, NY=33, NZ=17, pstrain_every=6, pressure_every=4)
    assert "pstrain_every = 6;" in c.to_string() and "pressure_every = 4;" in c.to_string()
    d = C.Config.from_string(c.to_string())
    assert (d.pstrain_every, d.pressure_every) == (6, 4)
    e = C.Config.from_string("NX = 32; NY = 33; NZ = 17; pstrain_every = 3;")
    assert (e.pstrain_every, e.pressure_every) == (3, 0)
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, pstrain_every=-1)
