"""Pressure strain on the GPU (Solver.static_pressure_hat: the pressure-mode export pass with the return
trip of p' to spectral space; Solver.pressure_strain: the Parseval reduction) against the NumPy
reference (reference/pressure.py) on the oracle's fields.

State and helpers as tests/test_pressure_gpu.py: random_state seed 9, amp 0.3, Re 400, parabolic U; for
fp32 storage the oracle is given the complex64-rounded phi and omega.  Tolerances are the project's own,
relative to the maximum of the compared field or row: 1e-9 in fp64, 1e-5 in fp32."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0


def _round32(a):
    return a.astype(np.complex64).astype(complex)


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32):
    """Oracle state (complex64-rounded for fp32 storage), its p-hat' [NY, nkx, nkz] and pressure-strain
    rows [7, NY]; computed once per case, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    if fp32:
        phi, om = _round32(phi), _round32(om)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    ph = prs.static_pressure_hat(o, prs.pressure_hat(o))
    rows = prs.pressure_strain(o, ph)
    for a in (phi, om, U, ph, rows):
        a.setflags(write=False)
    return dict(phi=phi, om=om, U=U, ph=ph, rows=rows)


def _solver(native, NX, NY, NZ, precision, **kw):
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=RE, precision=precision, ic="zero", log_every=0, symmetry_every=0,
                         **{"stats_every": 0, **kw})
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(NX, NY, NZ, precision == "fp32")
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s, ref


def _tol(precision):
    return 1e-9 if precision == "fp64" else 1e-5


def _check(s, ref, precision, what):
    """static_pressure_hat() against the reference p-hat' (the mean line exactly zero; the call itself
    refuses non-zero padding of the device layout) and pressure_strain() against the reference rows."""
    tol = _tol(precision)
    got = s.static_pressure_hat()
    want = ref["ph"]
    assert got.shape == want.shape and got.dtype == np.complex128 and np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: p-hat' rel. error {err:.3e} (tol {tol:.1e})")
    assert np.array_equal(got[:, 0, 0], np.zeros(got.shape[0], complex))
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"
    rows = s.pressure_strain()
    assert rows.shape == ref["rows"].shape and rows.dtype == np.float64 and np.isfinite(rows).all()
    for q, n in enumerate(prs.PSTRAIN_ROWS):
        e = np.abs(rows[q] - ref["rows"][q]).max() / np.abs(ref["rows"][q]).max()
        print(f"{what}: row {n} rel. error {e:.3e} (tol {tol:.1e})")
        assert e < tol, f"{what}: row {n} {e:.3e} >= {tol:.1e}"
    return got, rows


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_plain_layout(native, NX, precision):
    """R = 1, the plain layout, a non-power-of-two x length; lines = nkx * nkz is odd (a partial last tile)
    and the 48-row planes straddle the z blocks."""
    s, ref = _solver(native, NX, 33, 17, precision)
    assert s.spec_kzb() == 0
    _check(s, ref, precision, f"{NX}x33x17 {precision}")


def test_tiled_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 rows pad to 40."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check(s, ref, "fp64", "32x33x17 fp64 blocked")


@pytest.mark.parametrize("kzb", [0, 1])
def test_export_chunks(native, monkeypatch, kzb):
    """CHANNEL_YCHUNK=5: seven export chunks, a partial last one, chunk edges inside the 8-plane tiles:
    the forward x transform writes into a plane range of the spectral field."""
    monkeypatch.setenv("CHANNEL_YCHUNK", "5")
    monkeypatch.setenv("CHANNEL_SPEC_KZB", str(kzb))
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8 * kzb
    _check(s, ref, "fp64", f"32x33x17 fp64 ychunk 5 kzb {kzb}")


def test_r7_natural_tiled(native):
    s, ref = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    _check(s, ref, "fp32", "16x385x9 fp32 (R = 7)")


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("NZ", [513, 1025])
def test_long_rows(native, NZ, precision):
    """Nzp = 1024 (one wave per row in fp32) and 2048 (two waves per row: block barriers between the
    passes of the forward transform too)."""
    s, ref = _solver(native, 16, 17, NZ, precision)
    _check(s, ref, precision, f"16x17x{NZ} {precision}")


def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check(s, ref, "fp64", "32x33x17 fp64 combine")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_identities_on_the_device(native, precision):
    """Independently of the reference formulas: the Parseval rows pu and pv are the physical-space
    pressure_moments() rows 1 and 2 (u', v are band-limited), and the trace of rows 0 to 2 is zero
    (continuity), to the tolerance."""
    s, _ = _solver(native, 48, 33, 17, precision)
    tol = _tol(precision)
    rows = s.pressure_strain()
    pm = s.pressure_moments()
    for q, r in ((4, 1), (5, 2)):
        e = np.abs(rows[q] - pm[r]).max() / np.abs(pm[r]).max()
        print(f"{precision}: row {prs.PSTRAIN_ROWS[q]} against pressure_moments row {r}: rel. error {e:.3e} (tol {tol:.1e})")
        assert e < tol
    tr = np.abs(rows[0] + rows[1] + rows[2]).max() / np.abs(rows[:3]).max()
    print(f"{precision}: |ps_uu + ps_vv + ps_ww| / max row {tr:.3e} (tol {tol:.1e})")
    assert tr < tol


BALANCE_BOUNDS = (5e-3, 3e-2, 1e-3)  # (tests/test_pstrain_cpu.py: about three times the oracle's own error)


def test_component_energy_balance(native):
    """The CPU test's component balances on the solver itself (fp64): the <.> integrals from stats(),
    eps from gradient_sums(), the pressure-strain rows from pressure_strain(); central difference over
    two steps of dt = 1e-3 about the middle state."""
    dt = 1e-3
    cfg = default_config(NX=32, NY=65, NZ=17, Re=100.0, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=1, dt_fixed=dt)
    s = native.Solver(cfg, 0, 1, 0, b"")
    plan = ora.OraclePlan(32, 65, 17)
    ops = ora.build_ops(65)
    phi, om = bud.smooth_state(plan, ops, seed=3, amp=0.3, kscale=4)
    s.set_state(phi, om, 0.75 * 1.8 * (1 - ops.y ** 2))
    s.prepare()
    E = lambda: ops.trap @ np.asarray(s.stats()).reshape(4, 65)[:3].T  # noqa: E731
    E0 = E()
    s.step(True)
    st = np.asarray(s.stats()).reshape(4, 65)
    g = s.gradient_sums()
    ps = s.pressure_strain()
    U = np.asarray(s.mean_profile())
    prod = np.array([ops.trap @ (-2.0 * st[3] * (ops.D1 @ U)), 0.0, 0.0])
    eps = np.array([ops.trap @ (2.0 / 100.0 * g[3 + c]) for c in range(3)])
    pst = np.array([ops.trap @ ps[c] for c in range(3)])
    s.step(True)
    dE = (E() - E0) / (2 * dt)
    for c, name in enumerate(("uu", "vv", "ww")):
        err = abs(dE[c] - (prod[c] - eps[c] + pst[c])) / eps[c]
        half = abs(dE[c] - (prod[c] - eps[c] + 0.5 * pst[c])) / eps[c]
        print(f"{name}: dE/dt {dE[c]:.6e} P {prod[c]:.6e} eps {eps[c]:.6e} ps {pst[c]:.6e}  |difference| / eps {err:.2e} "
              f"(bound {BALANCE_BOUNDS[c]:.0e}); half the term {half:.2e}")
        assert err < BALANCE_BOUNDS[c], name
        assert half >= 10 * BALANCE_BOUNDS[c], name


DT = 1e-3


def _stepping_solver(native, **kw):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=2, dt_fixed=DT, **kw)
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(32, 33, 17, False)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s


def test_calls_do_not_disturb_the_run(native, tmp_path):
    """State, log and mean profile after 4 + 4 steps with both calls in between, each twice, are bitwise
    those of 8 undisturbed steps; static_pressure_hat is bitwise repeatable, the rows (atomics) to 1e-12;
    pressure_hat(), pressure_moments() and physical_fields(["p"]) are bitwise the same before and after
    the new calls on the same solver (pressure_moments to the 1e-12 of its atomics)."""
    a = _stepping_solver(native, path=str(tmp_path) + "/a_")
    a.run(8, False)
    b = _stepping_solver(native, path=str(tmp_path) + "/b_")
    b.run(4, False)
    st_before = np.asarray(b.stats()).copy()
    Pi1 = b.pressure_hat()
    m1 = b.pressure_moments()
    f1 = b.physical_fields([0, 5, 32], ["p"])["p"]
    P1 = b.static_pressure_hat()
    r1 = b.pressure_strain()
    P2 = b.static_pressure_hat()
    r2 = b.pressure_strain()
    assert np.array_equal(P1, P2)  # repeatable, bitwise
    d = np.abs(r2 - r1).max(axis=1) / np.abs(r1).max(axis=1)
    print(f"pressure_strain() twice: max |difference| / row max {d.max():.2e}")
    assert (d <= 1e-12).all()
    assert np.array_equal(b.pressure_hat(), Pi1)
    assert np.abs(b.pressure_moments() - m1).max() <= 1e-12 * np.abs(m1).max()
    assert np.array_equal(b.physical_fields([0, 5, 32], ["p"])["p"], f1)
    assert np.array_equal(np.asarray(b.stats()), st_before)
    b.run(4, False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    for k in ("step", "time", "dt", "umax", "vmax", "wmax", "cflsum", "dUdy_lo", "dUdy_hi", "flux", "dpdx", "utau", "health"):
        assert getattr(La, k) == getattr(Lb, k), k
    assert np.array_equal(np.asarray(a.mean_profile()), np.asarray(b.mean_profile()))


def test_one_rank_communicator_is_refused(native, monkeypatch, tmp_path, capfd):
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="random", ic_amplitude=0.1, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/", pstrain_every=2)
    assert c.solver.comm_kind() != "none"
    c.initialize()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.static_pressure_hat()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.pressure_strain()
    capfd.readouterr()
    c.run(4, False)
    err = capfd.readouterr().err
    assert err.count("pstrain_every") == 1 and "skipped" in err
    assert c.log().step == 4
    assert not list(tmp_path.glob("PS_*.dat"))


def test_files_and_sampled_profiles(native, tmp_path):
    Re = 1000.0
    cfg = default_config(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", pstrain_every=2)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    m = s.pressure_strain()
    for q, name in enumerate(("PS_UU", "PS_VV", "PS_WW", "PS_UV")):
        rows = np.loadtxt(tmp_path / f"{name}.dat")
        assert rows.shape == (2, 33) and np.isfinite(rows).all(), name
        # (nine significant digits in the files; the sums are atomics, equal to rounding only)
        assert np.abs(rows[1] - m[q]).max() <= 2e-8 * np.abs(m[q]).max(), name

    from channel_gpu_amd.models.channel import ChannelFlow
    from channel_gpu_amd.models.statistics import PSTRAIN_TERMS

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
    c.initialize()
    p = c.sample_statistics(8, every=2, budgets=True, pressure=True, pressure_strain=True).profiles()
    assert c.statistics.nps == 4
    for k in list(PSTRAIN_TERMS) + ["closure_uu", "closure_vv", "closure_ww", "closure_uv"]:
        assert k in p and p[k].shape == (17,) and np.isfinite(p[k]).all(), k
    assert np.abs(p["pstrain_uu"]).max() > 0
