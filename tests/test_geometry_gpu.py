"""Every device path that reads the box (ax = 2 pi / LX, az = 2 pi / LZ), the grid stretching or the
flow rate, on a geometry where a dropped, defaulted, squared-once-too-few or swapped factor shows:
GEOM_A = (LX 8 pi / 3, LZ 5 pi / 4, stretch 1.6, Q 1.3), ax = 0.75, az = 1.6, and the production box
GEOM_B = 4 pi x 2 pi (geomchecks.py).  test_geometry_cpu.py holds the precondition of every comparison
here: the NumPy reference itself moves by >= 1e-2 when the box is defaulted or swapped, the stretch or
Q defaulted.  test_multirank_gpu.py adds the slab and pencil ranks, test_kernels_gpu.py and
test_timestep_gpu.py the kernel-level cases.

No tolerance is new: each comparison uses the metric and the bound of the default-box test of the same
quantity, named where it is used."""
import os
import subprocess
import sys

import numpy as np
import pytest

import geomchecks as gc
import refchecks as rc
import test_budgets_gpu as t_bud
import test_pdfs_gpu as t_pdf
import test_physfields_gpu as t_phys
import test_sbudget_gpu as t_sb
import test_timestep_gpu as t_dt
import test_ycross_gpu as t_yc
import test_yspectra_gpu as t_ys
from channel_gpu_amd.models import orr_sommerfeld as osm
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pdfs as rp
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.reference import spectra as spc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


# ---- 3.1 whole steps against the oracle ---------------------------------------------------------------
def step_tolerances(precision, NY):
    """test_solver_gpu.py::test_gpu_matches_oracle_fp64 / _large_ny: relative L2 of phi, omega, U.
    Measured on the MI355X over the three steps (phi, omega, U): fp64 <= 3.7e-14, 1.8e-14, 5.1e-15 at
    32 x 33 x 17 (either geometry, either layout, combine mode) and 2.5e-13, 6.3e-12, 6.6e-12 at NY = 633;
    fp32 6.9e-6, 2.9e-6, 1.4e-6 at 32 x 33 x 17 and 1.6e-6, 2.0e-5, 6.9e-6 at NY = 385 (split K-SPEC:
    2.3e-6, 1.9e-5, 6.5e-6; its plane statistics <= 1.1e-5 against refchecks.stats_tol = 2e-4)."""
    return (1e-9, 1e-9, 1e-11) if precision == "fp64" else (1e-4 * max(1.0, NY / 600), 1e-4 * max(1.0, NY / 600), 1e-5)


def run_steps(native, grid, geom, precision, what):
    dt, state = gc.step_state(grid, geom, precision == "fp32")
    s = gc.make_solver(native, *grid, geom, precision, dt_fixed=dt)
    o = gc.make_oracle(*grid, geom, dt_fixed=dt)
    o.set_state(*state)
    s.set_state(*state)
    s.prepare()
    tol = step_tolerances(precision, grid[1])
    for it in range(gc.NSTEPS):
        o.step()
        s.step(False)
        gphi, gom, gU = s.get_state()
        e = rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U)
        print(f"GEOM_STEP {what} {precision} {grid} step {it}: rel err phi {e[0]:.3e} omega {e[1]:.3e} U {e[2]:.3e} "
              f"(tol {tol[0]:.1e} {tol[1]:.1e} {tol[2]:.1e})")
        assert e[0] < tol[0], f"phi step {it}: {e[0]:.3e}"
        assert e[1] < tol[1], f"omega step {it}: {e[1]:.3e}"
        assert e[2] < tol[2], f"U step {it}: {e[2]:.3e}"
    assert s.health() == 0
    if precision == "fp64":
        assert abs(o.ops.trap @ gU - gc.full(geom)["Q"]) < 1e-11  # (test_timestep_gpu.py::run_adaptive)
    # what the plan and the grid report (after the comparison: a wrong factor shall show in the numbers)
    p = s.plan
    assert abs(p.ax - o.plan.ax) < 1e-15 and abs(p.az - o.plan.az) < 1e-15
    assert np.abs(np.asarray(s.grid.y) - o.ops.y).max() < 1e-14
    return s


@pytest.mark.parametrize("geom,precision", [("A", "fp64"), ("A", "fp32"), ("B", "fp64")])
def test_steps_match_oracle(native, geom, precision):
    """32 x 33 x 17, R = 1, the plain layout, six K-SPEC outputs."""
    s = run_steps(native, gc.SMALL, gc.GEOM_A if geom == "A" else gc.GEOM_B, precision, f"GEOM_{geom}")
    assert s.spec_kzb() == 0 and not s.combine()


def test_steps_blocked_layout(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s = run_steps(native, gc.SMALL, gc.GEOM_A, "fp64", "blocked")
    assert s.spec_kzb() == 8


def test_steps_combine_mode(native, monkeypatch):
    """The x-backward combine gather (the P > 1 path) forms u, w, omega_x, omega_z with ax kx, az kz."""
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s = run_steps(native, gc.SMALL, gc.GEOM_A, "fp64", "combine")
    assert s.combine()


def test_steps_r7_blocked_by_default(native):
    s = run_steps(native, gc.R7, gc.GEOM_A, "fp32", "R = 7")
    assert s.spec_kzb() == 8


def test_steps_r10(native):
    run_steps(native, gc.R10, gc.GEOM_A, "fp64", "R = 10")


SPLIT_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHANNEL_ROOT"], "tests"))
import geomchecks as gc
import refchecks as rc
from channel_gpu_amd import require_native
C = require_native()
grid, precision, variant = gc.R7, "fp32", os.environ["SW_VARIANT"]
NY = grid[1]
dt, state = gc.step_state(grid, gc.GEOM_A, True)
s = gc.make_solver(C, *grid, gc.GEOM_A, precision, dt_fixed=dt, stats_every=1)
o = gc.make_oracle(*grid, gc.GEOM_A, dt_fixed=dt)
o.set_state(*state)
s.set_state(*state)
s.prepare()
o.prepare()
assert s.combine()
assert C.kspec_last_variant() == variant, C.kspec_last_variant()
rc.assert_stats_sensitive(o)
stol = rc.stats_tol(precision, NY)
tol, tolU = 1e-4 * max(1.0, NY / 600), 1e-5
e = rc.stats_errors(s.stats(), o.plane_stats())
print("GEOM_SPLIT prepare stats", e)
assert max(e) < stol, ("prepare()", e)
rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
for it in range(gc.NSTEPS):
    o.step()
    s.step(True)
    assert C.kspec_last_variant() == variant, C.kspec_last_variant()
    gphi, gom, gU = s.get_state()
    es = rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U)
    e = rc.stats_errors(s.stats(), o.plane_stats())
    print("GEOM_SPLIT step", it, "stats", e, "state", es)
    assert es[0] < tol and es[1] < tol and es[2] < tolU, (it, es)
    assert max(e) < stol, ("step(True)", it, e)
assert s.health() == 0
print("GEOM_SPLIT_OK")
"""


def test_steps_split_output_kernel():
    """CHANNEL_KSPEC_SPLIT=1 in the combine mode, fp32, NY = 385, in a child process as
    test_switches_gpu.py::test_kspec_split_matches_oracle: kspec_out_kernel has a wavenumber line of
    its own, which enters only the plane statistics, so those are compared at every step
    (refchecks.stats_tol) beside the state (the fp32 bounds of test_gpu_matches_oracle_large_ny)."""
    variant = "kspec_kernel<7, float, 4, 2, 2, 0, 0, 1, 1> + kspec_out_kernel<7, float, 8, 2>"
    env = dict(os.environ, CHANNEL_ROOT=ROOT, SW_VARIANT=variant, CHANNEL_KSPEC_SPLIT="1", CHANNEL_COMBINE="1")
    r = subprocess.run([sys.executable, "-c", SPLIT_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "GEOM_SPLIT_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- 3.2 time-step control ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_adaptive_dt_matches_oracle(native, precision):
    """test_timestep_gpu.py::test_adaptive_dt_matches_oracle on GEOM_A: its run_adaptive, so the four
    logged maxima and dt at refchecks.TOL_*, assert_cfl_sensitive on every pre-step state (cx = ax Kx,
    cz = az Kz from the oracle's plan), the state, the wall shear and the flux constraint at Q = 1.3."""
    _, state = gc.step_state(gc.SMALL, gc.GEOM_A, precision == "fp32")
    s = gc.make_solver(native, *gc.SMALL, gc.GEOM_A, precision, **gc.ADAPTIVE)
    o = gc.make_oracle(*gc.SMALL, gc.GEOM_A, **gc.ADAPTIVE)
    t_dt.run_adaptive(s, o, state, precision)
    assert s.graph_active()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_cfl_mode_parity(native, precision):
    """test_timestep_gpu.py::test_cfl_mode_parity on GEOM_A: dt, dt_c, dt_v at its 1e-6 against
    refchecks.dt_reference called with the configuration's LX, LZ; the state at the step tolerance."""
    NX, NY, NZ = gc.SMALL
    _, state = gc.step_state(gc.SMALL, gc.GEOM_A, precision == "fp32")
    cfg = gc.make_config(NX, NY, NZ, gc.GEOM_A, precision, cfl_mode="parity", **gc.ADAPTIVE)
    s = native.Solver(cfg, 0, 1, 0, b"")
    o = gc.make_oracle(NX, NY, NZ, gc.GEOM_A, **gc.ADAPTIVE)
    o.set_state(*state)
    s.set_state(*state)
    s.prepare()
    o.prepare()
    tol = step_tolerances(precision, NY)
    for it in range(2):
        t_dt.oracle_prestep_checks(o)
        s.step(False)
        L = s.log()
        o.dt_fixed = L.dt
        o.step()
        dt_c, dt_v, dt = rc.dt_reference(o.maxima, 0.5, 0.05, 0.0, 1, NX, NZ, cfg.LX, cfg.LZ, gc.RE, NY)
        print(f"parity step {it}: dt {L.dt} dt_c {L.dt_c} dt_v {L.dt_v}; reference {dt} {dt_c} {dt_v}")
        # fp32 storage: the plain maxima behind dt_c are held to TOL_CFL_F32 = 1e-4; dt_v is a formula
        tc = 1e-6 if precision == "fp64" else rc.TOL_CFL_F32
        for g, w_, what, t in ((L.dt, dt, "dt", tc), (L.dt_c, dt_c, "dt_c", tc), (L.dt_v, dt_v, "dt_v", 1e-6)):
            assert abs(g - w_) < t * w_, (what, g, w_)
        # (precondition) the parity step is not the corrected one
        assert abs(dt - min(o.cfl / o.maxima[3], o.dt_max)) > 1e-3 * dt
        assert rel(s.get_state()[0], o.phi) < tol[0]


# ---- 3.3 diagnostics --------------------------------------------------------------------------------------
def diag_solver(native, precision="fp64", **kw):
    ref = gc.diagnostics_reference(precision == "fp32")
    s = gc.make_solver(native, *gc.SMALL, gc.GEOM_A, precision,
                       **{"spectra_planes": ", ".join(map(str, gc.SPECTRA_PLANES)), "stats_every": 1, **kw})
    s.set_state(*ref["state"])
    s.prepare()
    return s, ref


@pytest.fixture(scope="module")
def diag(native):
    """One fp64 solver and one oracle on GEOM_A at 32 x 33 x 17 for all the fp64 diagnostics."""
    return diag_solver(native)


def test_diag_plane_stats(diag):
    s, ref = diag
    e = rc.stats_errors(s.stats(), ref["stats"])  # test_statistics_gpu.py
    print("stats() rows", e)
    assert max(e) < rc.stats_tol("fp64", gc.SMALL[1]), e


def check_spectra(s, ref, tol):
    """test_spectra_gpu.py::test_spectra_match_numpy."""
    sp = s.spectra()
    assert list(sp["planes"]) == list(gc.SPECTRA_PLANES)
    ekx, ekz, m = ref["spec_ekx"], ref["spec_ekz"], ref["spec_map"]
    assert np.allclose(sp["ekx"], ekx, rtol=tol, atol=tol * ekx.max())
    assert np.allclose(sp["ekz"], ekz, rtol=tol, atol=tol * ekz.max())
    assert np.allclose(sp["ekx"].sum(-1), sp["ekz"].sum(-1), rtol=1e-9)
    assert np.allclose(sp["map"], m, rtol=tol, atol=tol * m.max())


def test_diag_spectra(diag):
    check_spectra(*diag, 1e-10)


def test_diag_spectra_combine_mode(native, monkeypatch):
    """(1e-9: the combine mode's bound in every diagnostics file, e.g. test_yspectra_gpu.py)"""
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = diag_solver(native)
    assert s.combine()
    check_spectra(s, ref, 1e-9)


def test_diag_gradient_sums_and_transport(diag):
    s, ref = diag
    t_bud._check_rows(s.gradient_sums(), ref["grad"], 1e-10, bud.GRADIENT_ROWS, "gradient")
    t_bud._check_rows(s.transport_moments(), ref["tri"], 1e-10, bud.TRANSPORT_ROWS, "transport")


def check_max(got, want, tol, what):
    """Largest error relative to the maximum of the reference (test_pressure_gpu.py, test_pstrain_gpu.py)."""
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: rel. error {err:.3e} (tol {tol:.1e})")
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"


def test_diag_pressure(diag):
    """pressure_hat, pressure_moments, the p' planes, static_pressure_hat and pressure_strain at the 1e-9
    of test_pressure_gpu.py and test_pstrain_gpu.py."""
    s, ref = diag
    Pi = s.pressure_hat()
    assert np.array_equal(Pi[:, 0, 0], np.zeros(Pi.shape[0], complex))
    check_max(Pi, ref["Pi"], 1e-9, "Pi")
    pm = s.pressure_moments()
    for r, n in enumerate(prs.PRESSURE_ROWS):
        check_max(pm[r], ref["pmom"][r], 1e-9, f"pressure moment {n}")
    planes = [0, 5, 32]
    p = s.physical_fields(planes, ["p"])["p"]
    err = np.abs(p - ref["pp"][planes]).max() / np.abs(ref["pp"]).max()
    print(f"p' planes: rel. error {err:.3e}")
    assert err < 1e-9
    ph = s.static_pressure_hat()
    assert np.array_equal(ph[:, 0, 0], np.zeros(ph.shape[0], complex))
    check_max(ph, ref["p_hat"], 1e-9, "p-hat'")
    rows = s.pressure_strain()
    for q, n in enumerate(prs.PSTRAIN_ROWS):
        check_max(rows[q], ref["pstrain"][q], 1e-9, f"pressure strain {n}")


def check_plane_spectra(s, ref, tol, what):
    t_ys._check(s.plane_spectra(), dict(ekx=ref["ysp_ekx"], ekz=ref["ysp_ekz"]), tol, what)


def test_diag_plane_spectra(diag):
    """test_yspectra_gpu.py: rows 0 .. 6 at 1e-10; the pressure row as test_pressure_row, against the
    reference spectrum of the device's own p-hat' (itself compared in test_diag_pressure)."""
    s, ref = diag
    check_plane_spectra(s, ref, 1e-10, "GEOM_A")
    sp = s.plane_spectra(pressure=True)
    want = spc.plane_spectra(ref["o"], s.static_pressure_hat())
    t_ys._check(sp, want, 1e-10, "GEOM_A pressure", rows=[7])
    assert np.abs(want["ekx"][7]).max() > 0
    # (the oracle's own pp row, whose precondition test_geometry_cpu.py holds, is the same one)
    assert np.abs(want["ekx"][7] - ref["ysp_ekx"][7]).max() < 1e-8 * np.abs(ref["ysp_ekx"][7]).max()


def test_diag_plane_cross_spectra(diag):
    s, ref = diag
    for rows in ("velocity", "shear"):
        t_yc._check(s.plane_cross_spectra(list(gc.CROSS_REFS), rows), ref[f"cross_{rows}"], 1e-10, f"GEOM_A {rows}")


def test_diag_spectral_budgets(diag):
    s, ref = diag
    r = dict(H=ref["H"], ekx=ref["sb_ekx"], ekz=ref["sb_ekz"])
    t_sb._check_inputs(s, r, 1e-10, "GEOM_A")  # rotational_hat
    sb = s.spectral_budgets()
    U = ref["state"][2]
    assert np.abs(sb["U"] - U).max() < 1e-10 and np.abs(sb["dU"] - ref["o"].ops.D1 @ sb["U"]).max() < 1e-12
    t_sb._check(sb, r, 1e-10, "GEOM_A")


def test_diag_physical_fields_and_moments(diag):
    """test_physfields_gpu.py: all six fields at every plane, the eleven moments, 1e-10."""
    s, ref = diag
    NX, NY, NZ = gc.SMALL
    f = s.physical_fields(list(range(NY)), list(gc.NAMES))
    for i, n in enumerate(gc.NAMES):
        assert f[n].shape == (NY, NX, 2 * NZ - 2)
        t_phys._check(f[n], ref["phys"][i], 1e-10, n)
    U = ref["state"][2]
    assert np.abs(f["u"].mean(axis=(1, 2)) - U).max() < 1e-10 * np.abs(U).max()
    m = s.plane_moments()
    assert m.shape == (11, NY)
    for r in range(1, 11):
        check_max(m[r], ref["moments"][r], 1e-10, f"moment row {r}")
    assert np.abs(m[0]).max() <= 1e-10 * np.abs(U).max()


def test_diag_plane_histograms(diag):
    """test_pdfs_gpu.py::test_oracle_fields and ::test_wall_shear, both against the oracle's fields:
    the mid planes of all six fields, and omega_x, omega_z on the wall planes (the wall shear)."""
    s, ref = diag
    ph, tol = ref["phys"], 1e-10
    for planes, names in ((t_pdf.MID, list(gc.NAMES)), ([0, gc.SMALL[1] - 1], ["wx", "wz"])):
        h = t_pdf._hist(s, planes, nbins=32, njoint=16, span=4.0, vorticity=True)
        assert list(h["names"]) == list(gc.NAMES)
        fields = {n: ph[gc.NAMES.index(n)][planes] for n in names}
        deltas = {n: np.full(len(planes), tol * np.abs(ph[gc.NAMES.index(n)]).max()) for n in names}
        t_pdf._compare(h, fields, names, deltas)
        if "u" in names:
            t_pdf._check_marginals(h)
        # the default centre of omega_z is -D1 U: the plane mean of the reference field
        err = np.abs(h["centre"][5] - ph[5][planes].mean(axis=(1, 2))).max() / np.abs(ph[5]).max()
        print(f"centre of wz against the oracle's plane mean: {err:.2e}")
        assert err < tol


def test_diag_fp32(native):
    """fp32 storage (two elements per lane) once, for gradient_sums and plane_spectra: 1e-5."""
    s, ref = diag_solver(native, "fp32")
    t_bud._check_rows(s.gradient_sums(), ref["grad"], 1e-5, bud.GRADIENT_ROWS, "gradient fp32")
    check_plane_spectra(s, ref, 1e-5, "GEOM_A fp32")


def test_diag_blocked_layout(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = diag_solver(native)
    assert s.spec_kzb() == 8
    check_plane_spectra(s, ref, 1e-10, "GEOM_A blocked")
    r = dict(H=ref["H"], ekx=ref["sb_ekx"], ekz=ref["sb_ekz"])
    t_sb._check_inputs(s, r, 1e-10, "GEOM_A blocked")
    t_sb._check(s.spectral_budgets(), r, 1e-10, "GEOM_A blocked")


# ---- 3.4 physics, independent of the oracle ------------------------------------------------------------
def test_ts_wave_growth_rate_long_box(native):
    """test_physics_gpu.py::test_ts_wave_growth_rate with LX = 4 pi and the wave at kx index 2 (NX = 16
    retains |kx| <= 5): alpha = ax * 2 = 1 again, so the Orr-Sommerfeld eigenvalue and the 1 % band
    are that test's.  A solver that ignored ax would advance an alpha = 2 wave, which decays."""
    NX, NY, NZ, Re, dt = 16, 129, 9, 7500.0, 0.02
    LX = gc.GEOM_B["LX"]
    from channel_gpu_amd.utils.config import default_config

    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=Re, Q=4.0 / 3.0, LX=LX, precision="fp64", dt_fixed=dt, ic="zero",
                         stats_every=0, log_every=0, symmetry_every=0)
    s = native.Solver(cfg, 0, 1, 0, b"")
    plan = ora.OraclePlan(NX, NY, NZ, LX=LX)
    ops = ora.build_ops(NY)
    phi, om, U, c = osm.ts_initial_state(plan, ops, Re, eps=1e-6, alpha_index=2)
    assert abs(plan.ax * 2 - 1.0) < 1e-15
    s.set_state(phi, om, U)
    s.prepare()
    amps, ts = [], []
    for i in range(1500):
        s.step(False)
        if i % 250 == 249:
            p, _, _ = s.get_state()
            amps.append(np.linalg.norm(p[:, 2, 0]))
            ts.append((i + 1) * dt)
    rates = np.diff(np.log(amps)) / np.diff(ts)
    sigma = c.imag  # alpha = 1
    assert np.all(np.abs(rates - sigma) < 0.01 * sigma), (rates, sigma)
    assert s.health() == 0


# ---- the random initial condition -------------------------------------------------------------------------
def test_random_ic_envelope_follows_the_box(native):
    """ic = "random" has no NumPy twin, but its draws depend on (seed, |kx|, kz) alone and its envelope
    is exp(-k2 / 32): between two boxes on the same y grid every omega line scales by
    exp(-(k2_A - k2_default) / 32) (two exp and a product: held to 100 ulp), and U is 0.75 Q (1 - y^2)."""
    NX, NY, NZ = gc.SMALL
    box = dict(stretch=gc.GEOM_A["stretch"], Q=gc.GEOM_A["Q"])
    res = []
    for geom in (gc.GEOM_A, box):
        s = gc.make_solver(native, NX, NY, NZ, geom, "fp64", ic="random", ic_amplitude=0.3)
        s.init_ic()
        res.append(s.get_state())
    (_, om_a, U_a), (_, om_d, _) = res
    pa, pd = gc.make_oracle(NX, NY, NZ, gc.GEOM_A), gc.make_oracle(NX, NY, NZ, box)
    ratio = lambda a, d: np.exp(-(a.k2 - d.k2) / 32.0).reshape(om_a.shape[1:])  # noqa: E731
    r = ratio(pa, pd)
    err = np.abs(om_a - r * om_d).max() / np.abs(om_a).max()
    print(f"random IC: omega_A against the rescaled default-box omega: {err:.2e}")
    assert np.abs(om_a).max() > 0 and err < 100 * np.finfo(float).eps
    # (precondition) a swapped or defaulted box would give another envelope
    for name in gc.BOX:
        g = gc.mutated(gc.GEOM_A, name)
        d = np.abs(ratio(ora.OracleSolver(NX, NY, NZ, **g), pd) * om_d - om_a).max() / np.abs(om_a).max()
        assert d >= gc.SENSITIVITY, (name, d)
    assert np.abs(U_a - 0.75 * gc.GEOM_A["Q"] * (1 - pa.ops.y ** 2)).max() < 1e-14


# ---- 3.6 the Python wrapper ----------------------------------------------------------------------------------
def test_wrapper_wavenumber_axes(native):
    from channel_gpu_amd.models.channel import ChannelFlow

    NX, NY, NZ = gc.SMALL
    ref = gc.diagnostics_reference()
    c = ChannelFlow(gc.make_config(NX, NY, NZ, gc.GEOM_A, "fp64"))
    c.set_state(*ref["state"])
    p = ref["o"].plan
    kx, kz = 0.75 * np.arange(p.Kx + 1), 1.6 * np.arange(p.nkz)
    assert c.statistics.stretch == gc.GEOM_A["stretch"]
    c.statistics._ops()  # (raises on another stretch than the grid's)
    for what, d in (("plane_spectra", c.plane_spectra(pressure=True)),
                    ("plane_cross_spectra", c.plane_cross_spectra(list(gc.CROSS_REFS))),
                    ("spectral_budgets", c.spectral_budgets())):
        assert np.allclose(d["kx"], kx, rtol=1e-15, atol=0) and np.allclose(d["kz"], kz, rtol=1e-15, atol=0), what
    check_plane_spectra(c, ref, 1e-10, "wrapper")
