"""NumPy reference of the spectral Reynolds-stress budgets (reference/spectral_budgets.py) on the oracle:
closure of the four budgets per mode over one oracle step, Parseval against physical space, consistency
with the plane sums the project already has, the wall-unit averaging of TurbulenceStatistics and the
config key.  No GPU.

Closure: 16 x NY x 9, Re = 400, smooth_state(seed=9, amp=0.3), U = 0.75 * 1.8 * (1 - y^2), one oracle step
of dt = 1e-6; the residual is rate - RHS per mode over rows [2:-2] and k2 > 0, relative to the largest
term of the budget over the same set.  Measured:

    NY     uu       vv       ww       uv
    65   3.5e-2   4.1e-3   2.5e-2   1.9e-3
   129   1.9e-3   1.7e-4   9.4e-4   2.3e-4

(the truncation error of the compact operators on products of the fields; it falls 10 to 25 times from
NY = 65 to 129).  With one term of the right-hand side removed (the production, the n, the gs or the
D1(g.) term) the residual is 0.19 (the production of uv) to 1.0.  The two viscous terms are not part of
that check: at Re = 400 they are 0.01 to 0.26 of the largest term; the g rows they are made of are
checked against the gradient sums."""
import copy
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import SBUDGET_ROWS, SBUDGET_STRESSES, SBUDGET_TERMS, TurbulenceStatistics
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.reference import spectral_budgets as sbr

RE = 400.0
DT = 1e-6
ROW = sbr.ROW


def _oracle(NX, NY, NZ, smooth=True, **kw):
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE, **kw)
    make = bud.smooth_state if smooth else ora.random_state
    phi, om = make(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    return o


def _equations(o, rows, E):
    """The right-hand sides of the four budgets as lists of terms [NY, lines]; the last two are viscous."""
    r = {n: rows[i] for n, i in ROW.items()}
    D1, D2, nu = o.ops.D1, o.ops.D2, o.nu
    dU = (D1 @ o.U)[:, None]
    visc = lambda i, s: [nu * (D2 @ E[i]), -2.0 * nu * r["g_" + s]]  # noqa: E731
    return {"uu": [-2.0 * dU * E[3], 2.0 * r["n_uu"], r["gs_uu"]] + visc(0, "uu"),
            "vv": [2.0 * r["n_vv"], r["gs_vv"], -2.0 * (D1 @ r["gv"])] + visc(1, "vv"),
            "ww": [2.0 * r["n_ww"], r["gs_ww"]] + visc(2, "ww"),
            "uv": [-dU * E[1], r["n_uv"], r["gs_uv"], -(D1 @ r["gu"])] + visc(3, "uv")}


@functools.lru_cache(maxsize=None)
def _closure(NY):
    """{stress: [residual, residual without term 0, without term 1, ...]} (the viscous terms last)."""
    o = _oracle(16, NY, 9, dt_fixed=DT)
    rows, E0 = sbr.mode_rows(o), sbr.stress_rows(o)
    eq = _equations(o, rows, E0)
    o1 = copy.deepcopy(o)
    o1.step()
    if o1.fields is None:
        o1.prepare()
    rate = (sbr.stress_rows(o1) - E0) / DT
    keep = o.k2 > 0
    sel = lambda a: a[2:-2][:, keep]  # noqa: E731
    out = {}
    for i, s in enumerate(SBUDGET_STRESSES):
        terms = eq[s]
        big = max(np.abs(sel(t)).max() for t in terms)
        out[s] = [np.abs(sel(rate[i] - sum(t for k, t in enumerate(terms) if k != d))).max() / big
                  for d in [None] + list(range(len(terms)))]
    return out


def test_closure_per_mode():
    c65, c129 = _closure(65), _closure(129)
    for s in SBUDGET_STRESSES:
        print(f"{s}: residual {c65[s][0]:.2e} (NY = 65), {c129[s][0]:.2e} (NY = 129); one term removed "
              + " ".join(f"{x:.3f}" for x in c129[s][1:]))
        assert c129[s][0] < 5e-3, (s, c129[s][0])
        assert c65[s][0] > 3.0 * c129[s][0], (s, c65[s][0], c129[s][0])
        for c in (c65, c129):
            for x in c[s][1:-2]:  # (every term but the two viscous ones)
                assert x > 0.1, (s, c[s])


def test_terms_sum_to_the_rate():
    """budget_terms regroups the same right-hand side (production, nonlinear, pressure strain, pressure
    diffusion, viscous diffusion, dissipation): same closure."""
    o = _oracle(16, 129, 9, dt_fixed=DT)
    rows, E0 = sbr.mode_rows(o), sbr.stress_rows(o)
    T = sbr.budget_terms(o.ops, o.nu, o.U, rows, E0)
    eq = _equations(o, rows, E0)
    keep = o.k2 > 0
    for s in SBUDGET_STRESSES:
        assert tuple(T[s]) == SBUDGET_TERMS[:-1]
        a, b = sum(T[s].values())[:, keep], sum(eq[s])[:, keep]
        assert np.abs(a - b).max() < 1e-12 * max(np.abs(t[:, keep]).max() for t in eq[s]), s


@functools.lru_cache(maxsize=None)
def _case():
    o = _oracle(32, 33, 17, smooth=False)
    Pi = prs.pressure_hat(o)
    ph = prs.static_pressure_hat(o, Pi)
    sb = sbr.spectral_budgets(o, Pi=Pi, p_hat=ph)
    return o, ph, sb


def _close(a, b, tol, what, scale=None):
    err = np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale)
    print(f"{what}: {err:.2e}")
    assert err < tol, (what, err)


def test_rows_and_shapes():
    o, _, sb = _case()
    p = o.plan
    assert tuple(sb["rows"]) == SBUDGET_ROWS == sbr.SBUDGET_ROWS and len(SBUDGET_ROWS) == 20
    assert sb["ekx"].shape == (20, 33, p.Kx + 1) and sb["ekz"].shape == (20, 33, p.nkz)
    assert np.array_equal(sb["dU"], o.ops.D1 @ o.U)
    for r in range(20):
        assert np.abs(sb["ekx"][r]).max() > 0, SBUDGET_ROWS[r]
        _close(sb["ekx"][r].sum(-1), sb["ekz"][r].sum(-1), 1e-12, f"k-sums of {SBUDGET_ROWS[r]}", np.abs(sb["ekx"][r]).max())


def test_parseval_against_physical_space():
    o, _, sb = _case()
    phys = ora.spec_to_phys_full(o.fields, o.plan)
    f = phys.copy()
    f[0] -= o.U[:, None, None]
    f[5] += (o.ops.D1 @ o.U)[:, None, None]  # omega_z' = omega_z + U'
    h = ora.rotational_product(f)
    for c, name in enumerate(("n_uu", "n_vv", "n_ww")):
        want = (f[c] * h[c]).mean(axis=(1, 2))
        for e in ("ekx", "ekz"):
            _close(sb[e][ROW[name]].sum(-1), want, 1e-12, f"{e} {name} against physical space")
    want = (f[0] * h[1] + f[1] * h[0]).mean(axis=(1, 2))
    _close(sb["ekx"][ROW["n_uv"]].sum(-1), want, 1e-12, "ekx n_uv against physical space")


def test_consistency_with_the_plane_sums():
    o, ph, sb = _case()
    g = bud.gradient_sums(o)
    ps = prs.pressure_strain(o, ph)
    for e in ("ekx", "ekz"):
        for q in range(4):
            _close(sb[e][4 + q].sum(-1), g[3 + q], 1e-12, f"{e} {SBUDGET_ROWS[4 + q]} summed against gradient_sums")
        for q in range(6):
            _close(sb[e][14 + q].sum(-1), ps[q], 1e-12, f"{e} {SBUDGET_ROWS[14 + q]} summed against pressure_strain")
        big = np.abs(sb[e]).max(axis=(1, 2))
        for a in (8, 14):  # continuity: the traces of gs and ps vanish per bin
            assert np.abs(sb[e][a] + sb[e][a + 1] + sb[e][a + 2]).max() < 1e-12 * big[a:a + 3].max(), (e, a)


def test_statistics_of_synthetic_rows():
    """Rows with one known entry each: the terms are the arithmetic of the docstring, folded and in wall
    units, the premultiplied forms (k / dk) times them, and the residual minus the sum."""
    NY, nkx, nkz = 33, 4, 5
    ops = ora.build_ops(NY)
    nu, ut_lo, ut_hi = 1.0 / 180.0, 0.06, 0.07
    ut = np.sqrt(0.5 * (ut_lo ** 2 + ut_hi ** 2))
    rng = np.random.default_rng(3)
    U = 1.0 - ops.y ** 2
    S = TurbulenceStatistics(ops.y, nu)
    with pytest.raises(ValueError):
        S.spectral_budgets()
    bkx, bkz = rng.standard_normal((20, NY, nkx)), rng.standard_normal((20, NY, nkz))
    ekx, ekz = rng.standard_normal((4, NY, nkx)), rng.standard_normal((4, NY, nkz))
    kx, kz = 1.0 * np.arange(nkx), 2.0 * np.arange(nkz)
    for f in (1.0, 3.0):  # (two samples: the mean is twice the first)
        S.add(U, np.zeros(4 * NY), ut_lo, ut_hi, 0.0)
        S.add_spectral_budgets(f * bkx, f * bkz, f * ekx, f * ekz, kx, kz)
    assert S.nsb == 2
    r = S.spectral_budgets()
    h = (NY + 1) // 2
    lo, hi = np.arange(h), NY - 1 - np.arange(h)
    dU = (ops.D1 @ U)[:, None]
    d1 = lambda a: ops.D1 @ a  # noqa: E731
    sc = nu / ut ** 4
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)  # noqa: E731
    assert close(r["y_plus"], (1 + ops.y[lo]) * ut / nu) and close(r["kz_plus"], kz * nu / ut)
    assert np.isinf(r["lambda_x_plus"][0]) and close(r["lambda_z_plus"][1:], 2 * np.pi * ut / nu / kz[1:])
    for key, b, e, k in (("x", 2.0 * bkx, 2.0 * ekx, kx), ("z", 2.0 * bkz, 2.0 * ekz, kz)):
        R = {n: b[i] for n, i in ROW.items()}
        zero = np.zeros_like(e[0])
        want = {
            "uu": {"production": -2 * dU * e[3], "nonlinear": 2 * R["n_uu"] + R["gs_uu"] - R["ps_uu"],
                   "pressure_strain": R["ps_uu"], "pressure_diffusion": zero},
            "vv": {"production": zero, "nonlinear": 2 * R["n_vv"] + R["gs_vv"] - R["ps_vv"] - 2 * d1(R["gv"] - R["pv"]),
                   "pressure_strain": R["ps_vv"], "pressure_diffusion": -2 * d1(R["pv"])},
            "ww": {"production": zero, "nonlinear": 2 * R["n_ww"] + R["gs_ww"] - R["ps_ww"],
                   "pressure_strain": R["ps_ww"], "pressure_diffusion": zero},
            "uv": {"production": -dU * e[1], "nonlinear": R["n_uv"] + R["gs_uv"] - R["ps_uv"] - d1(R["gu"] - R["pu"]),
                   "pressure_strain": R["ps_uv"], "pressure_diffusion": -d1(R["pu"])},
        }
        for i, s in enumerate(SBUDGET_STRESSES):
            want[s]["viscous_diffusion"] = nu * (ops.D2 @ e[i])
            want[s]["dissipation"] = -2 * nu * R["g_" + s]
            want[s]["residual"] = -sum(want[s].values())
            got = r["terms_k" + key][s]
            assert tuple(got) == SBUDGET_TERMS
            sgn = -1.0 if s == "uv" else 1.0
            for t in SBUDGET_TERMS:
                w = sc * 0.5 * (want[s][t][lo] + sgn * want[s][t][hi])
                assert got[t].shape == (h, k.size) and close(got[t], w), (key, s, t)
                assert close(r["premult_k" + key][s][t], k / k[1] * w), (key, s, t)
    with pytest.raises(ValueError):
        S.add_spectral_budgets(bkx[:19], bkz[:19], ekx, ekz, kx, kz)
    with pytest.raises(ValueError):
        S.add_spectral_budgets(bkx, bkz, ekx[:3], ekz[:3], kx, kz)


def test_config_key():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    assert C.Config().sbudget_every == 0
    c = default_config(NX=32, NY=33, NZ=17, sbudget_every=6)
    assert c.sbudget_every == 6 and "sbudget_every = 6;" in c.to_string()
    assert C.Config.from_string(c.to_string()).sbudget_every == 6
    d = C.Config.from_string("NX = 32; NY = 33; NZ = 17; sbudget_every = 3;")
    assert d.sbudget_every == 3
    assert C.Config.from_string("NX = 32; NY = 33; NZ = 17;").sbudget_every == 0
    c.sbudget_every = 2
    assert c.sbudget_every == 2
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, sbudget_every=-1)
    with pytest.raises(RuntimeError):
        C.Config.from_string("NX = 32; NY = 33; NZ = 17; sbudget_every = -2;").validate()
