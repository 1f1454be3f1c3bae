"""Pressure on the CPU: the NumPy reference (reference/pressure.py) in the oracle's own momentum
equations, the pressure profiles of TurbulenceStatistics on synthetic sums, and the config keys."""
import copy
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import PRESSURE_ROWS, PRESSURE_TERMS, TurbulenceStatistics
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs

DT = 1e-6


@functools.lru_cache(maxsize=None)
def _residuals(NY):
    """One oracle step of dt = 1e-6 from a smooth state at 16 x NY x 9, Re = 400: the maxima over rows
    [2:-2] and the lines with k2 > 0 of the u, v, w momentum residuals with and without grad Pi, and
    the scales max |D1 Pi|, max |i al Pi|."""
    o = ora.OracleSolver(NX=16, NY=NY, NZ=9, Re=400.0, dt_fixed=DT)
    phi, om = bud.smooth_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    Pi = prs.pressure_hat(o)
    o1 = copy.deepcopy(o)
    o1.step()
    keep = o.k2 > 0
    mx = lambda a: float(np.abs(a[2:-2][:, keep]).max())  # noqa: E731
    with_p = tuple(mx(r) for r in prs.momentum_residual(o, Pi, o1, DT))
    without = tuple(mx(r) for r in prs.momentum_residual(o, np.zeros_like(Pi), o1, DT))
    scale_v = float(np.abs(o.ops.D1 @ Pi).max())
    scale_u = float(np.abs(o.al * Pi).max())
    assert np.array_equal(Pi[:, ~keep], np.zeros_like(Pi[:, ~keep]))  # the mean line
    return with_p, without, scale_v, scale_u


def test_momentum_residual_converges():
    """The reference Pi closes the oracle's v- and u-momentum equations to the y-discretisation's
    error.  Measured: v residual / max |D1 Pi| = 3.5e-3 (NY = 65), 6.0e-4 (NY = 129), ratio 5.8; u
    residual 8.2e-2 -> 1.4e-2; without grad Pi 1.0 of the scale."""
    r65, _, s65, _ = _residuals(65)
    r129, n129, s129, su129 = _residuals(129)
    print(f"NY=65 : u {r65[0]:.3e} v {r65[1]:.3e} w {r65[2]:.3e}  max|D1 Pi| {s65:.4f}")
    print(f"NY=129: u {r129[0]:.3e} v {r129[1]:.3e} w {r129[2]:.3e}  max|D1 Pi| {s129:.4f} max|i al Pi| {su129:.4f}")
    print(f"NY=129 without grad Pi: u {n129[0]:.3e} v {n129[1]:.3e} w {n129[2]:.3e}")
    assert r129[1] < 2e-3 * s129
    assert r65[1] > 3.0 * r129[1]
    assert r65[0] > 3.0 * r129[0]
    assert n129[1] > 0.5 * s129
    assert n129[0] > 0.5 * su129


def test_pressure_moments_match_the_physical_field():
    """pressure_moments row 0 is the plane variance of pressure_physical, whose planes have zero mean;
    <p'v> and <p'w> need no mean correction (v, w have none)."""
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    Pi = prs.pressure_hat(o)
    p = prs.pressure_physical(o, Pi)
    m = prs.pressure_moments(o, Pi)
    assert p.shape == (33, 32, 32) and m.shape == (4, 33)
    assert np.abs(p.mean(axis=(1, 2))).max() < 1e-14 * np.abs(p).max()
    assert np.abs(m[0] - p.var(axis=(1, 2))).max() < 1e-13 * m[0].max()
    v = ora.spec_to_phys_full(o.fields[1], o.plan)
    assert np.abs(m[2] - (p * v).mean(axis=(1, 2))).max() < 1e-13 * np.abs(m[2]).max()
    # Pi is Hermitian on kz = 0 (a real field): the transform to physical space loses nothing
    P = Pi.reshape(o.phi.shape)
    kx = np.arange(1, o.plan.Kx + 1)
    assert np.abs(P[:, kx, 0] - np.conj(P[:, o.plan.nkx - kx, 0])).max() < 1e-12 * np.abs(P).max()


@functools.lru_cache(maxsize=None)
def _synthetic(n=33):
    """One asymmetric synthetic sample (no parity in y)."""
    rng = np.random.default_rng(11)
    y = ora.ygrid(n)
    smooth = lambda: (1 - y ** 2) * (rng.uniform(-1, 1) + rng.uniform(-1, 1) * y + rng.uniform(-1, 1) * y ** 2 +  # noqa: E731
                                      rng.uniform(-1, 1) * y ** 3)
    U = 1.35 * (1 - y ** 2) * (1 + 0.1 * y)
    st = np.stack([smooth() ** 2 + 0.1 * (1 - y ** 2), smooth() ** 2, smooth() ** 2, smooth()])
    grad = np.stack([np.abs(smooth()) + 0.3 + 0.1 * y for _ in range(6)] + [smooth()])
    triple = np.stack([smooth() for _ in range(3)])
    pm = np.stack([smooth() ** 2 + 0.2 + 0.05 * y, smooth() + 0.1 * y, smooth(), smooth()])
    return y, U, st, grad, triple, smooth(), pm


def test_statistics_pressure_profiles():
    y, U, st, grad, triple, vvv, pm = _synthetic()
    n, nu = y.size, 1.0 / 180.0
    ops = ora.build_ops(n)
    S = TurbulenceStatistics(y, nu)
    with pytest.raises(ValueError):
        S.pressure_terms()
    ut_lo, ut_hi = 0.06, 0.07
    S.add(U, st.ravel(), ut_lo, ut_hi, 0.0)
    assert "p_rms" not in S.profiles()
    # two samples: the averages are formed first
    S.add_pressure(0.5 * pm)
    S.add_pressure(1.5 * pm)
    assert S.npr == 2 and PRESSURE_ROWS == ("pp", "pu", "pv", "pw")
    t = S.pressure_terms()
    ref = {"pdiff_k": -(ops.D1 @ pm[2]), "pdiff_vv": -2 * (ops.D1 @ pm[2]), "pdiff_uv": -(ops.D1 @ pm[1])}
    assert sorted(t) == sorted(PRESSURE_TERMS)
    for k, r in ref.items():
        assert np.abs(t[k] - r).max() <= 1e-12 * np.abs(r).max(), k
    p = S.profiles()
    assert "closure_k" not in p  # (needs the budgets)
    ut = np.sqrt(0.5 * (ut_lo ** 2 + ut_hi ** 2))
    h = (n + 1) // 2
    lo, hi = np.arange(h), n - 1 - np.arange(h)
    fold = lambda a, s: 0.5 * (a[lo] + s * a[hi])  # noqa: E731
    want = {"p_rms": (np.sqrt(fold(pm[0], 1.0)) / ut ** 2, None),
            "pu": (fold(pm[1], 1.0) / ut ** 3, fold(pm[1], -1.0) / ut ** 3),
            "pv": (fold(pm[2], -1.0) / ut ** 3, fold(pm[2], 1.0) / ut ** 3),
            "pdiff_k": (fold(ref["pdiff_k"], 1.0) * nu / ut ** 4, fold(ref["pdiff_k"], -1.0) * nu / ut ** 4),
            "pdiff_vv": (fold(ref["pdiff_vv"], 1.0) * nu / ut ** 4, fold(ref["pdiff_vv"], -1.0) * nu / ut ** 4),
            "pdiff_uv": (fold(ref["pdiff_uv"], -1.0) * nu / ut ** 4, fold(ref["pdiff_uv"], 1.0) * nu / ut ** 4)}
    for k, (w, other) in want.items():
        assert p[k].shape == (h,), k
        assert np.abs(p[k] - w).max() <= 1e-12 * np.abs(w).max(), k
        # (the asymmetric input tells the two parities apart)
        if other is not None:
            assert np.abs(p[k] - other).max() > 1e-6 * np.abs(w).max(), k
    # with the budgets: closure_k = resid_k - pdiff_k, and the existing keys keep their values
    S.add_budgets(grad, triple, vvv)
    q = S.profiles()
    assert np.array_equal(q["closure_k"], q["resid_k"] - q["pdiff_k"])
    S2 = TurbulenceStatistics(y, nu)
    S2.add(U, st.ravel(), ut_lo, ut_hi, 0.0)
    S2.add_budgets(grad, triple, vvv)
    q2 = S2.profiles()
    for k, a in q2.items():
        assert np.array_equal(a, q[k]), k
    assert sorted(set(q) - set(q2)) == sorted(["p_rms", "pu", "pv", "closure_k"] + list(PRESSURE_TERMS))


def test_statistics_write_appends_pressure_columns(tmp_path):
    y, U, st, grad, triple, vvv, pm = _synthetic()
    S = TurbulenceStatistics(y, 1.0 / 180.0)
    S.add(U, st.ravel(), 0.06, 0.07, 0.0)
    S.add_budgets(grad, triple, vvv)
    S.write(str(tmp_path / "a.dat"))
    base = np.loadtxt(tmp_path / "a.dat")
    S.add_pressure(pm)
    S.write(str(tmp_path / "b.dat"))
    full = np.loadtxt(tmp_path / "b.dat")
    assert full.shape == (base.shape[0], base.shape[1] + 7)
    names = (tmp_path / "b.dat").read_text().splitlines()[1].split()[1:]
    assert names[-7:] == ["p_rms", "pu", "pv", "pdiff_k", "pdiff_vv", "pdiff_uv", "closure_k"]
    assert np.allclose(full[:, names.index("closure_k")], S.profiles()["closure_k"], rtol=1e-6, atol=1e-12)


def test_config_keys():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    assert C.Config().pressure_every == 0
    c = default_config(NX=32, NY=33, NZ=17, pressure_every=6, fields="u,p")
    assert "pressure_every = 6;" in c.to_string()
    d = C.Config.from_string(c.to_string())
    assert (d.pressure_every, d.fields) == (6, "u,p")
    e = C.Config.from_string("NX = 32; NY = 33; NZ = 17; pressure_every = 3; fields = \"p\";")
    assert (e.pressure_every, e.fields) == (3, "p")
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, pressure_every=-1)
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, fields="u,q")
