"""The NumPy side of the non-default-geometry tests (geomchecks.py), without a GPU: every reference
that test_geometry_gpu.py and the GEOM_A cases of test_multirank_gpu.py compare against must itself
tell GEOM_A (GEOM_B) from the default box, from a swapped box, from the default stretch and from the
default flow rate, on the exact grids, seeds and step counts used there; the oracle on GEOM_A is
divergence-free and holds the flux Q; TurbulenceStatistics rebuilds its operators from the stretch."""
import numpy as np
import pytest

import geomchecks as gc
from channel_gpu_amd.models import orr_sommerfeld as osm
from channel_gpu_amd.models.statistics import TurbulenceStatistics
from channel_gpu_amd.reference import oracle as ora


def _report(what, moved):
    for name, d in moved.items():
        print(f"{what} | {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    return min(v for d in moved.values() for v in d.values())


def test_geometries_are_what_they_claim():
    a = gc.make_oracle(*gc.SMALL, gc.GEOM_A).plan
    vals = [a.ax, a.az, a.ax ** 2, a.az ** 2, a.ax * a.az, 1 / a.ax, 1 / a.az]
    assert abs(a.ax - 0.75) < 1e-15 and abs(a.az - 1.6) < 1e-15
    for i, v in enumerate(vals):
        assert all(abs(v - w) > 1e-3 for w in vals[:i] + [1.0, 2.0, 4.0]), vals
    b = gc.make_oracle(*gc.SMALL, gc.GEOM_B).plan
    assert abs(b.ax - 0.5) < 1e-15 and abs(b.az - 1.0) < 1e-15
    # GEOM_B keeps the default stretch and Q: those mutations do not apply to it
    assert gc.mutated(gc.GEOM_B, "stretch -> 2.0") is None and gc.mutated(gc.GEOM_B, "Q -> 1.8") is None
    assert all(gc.mutated(gc.GEOM_A, m) is not None for m in gc.MUTATIONS)


@pytest.mark.parametrize("case", list(gc.STEP_REFERENCES))
def test_step_references_feel_the_geometry(case):
    """Three steps: phi and omega move under every box mutation and the stretch, U also under Q."""
    grid, geom, fp32 = gc.STEP_REFERENCES[case]
    dt, state = gc.step_state(grid, geom, fp32)
    moved = gc.assert_geometry_sensitive(gc.steps, geom, state, gc.STEP_WHICH, grid, dt_fixed=dt)
    assert _report(case, moved) >= gc.SENSITIVITY
    want = 5 if geom is gc.GEOM_A else 3
    assert len(moved) == want and all(("U" in d) for d in moved.values())
    if geom is gc.GEOM_A:
        assert set(moved["Q -> 1.8"]) == {"U"}


def test_multirank_references_feel_the_geometry():
    m = gc.MULTIRANK
    state = gc.make_state(*m["grid"], gc.GEOM_A, m["seed"], m["amp"])
    moved = gc.assert_geometry_sensitive(lambda o: gc.steps(o, m["nsteps"]), gc.GEOM_A, state, gc.STEP_WHICH, m["grid"],
                                         dt_fixed=m["dt"])
    assert _report("multirank", moved) >= gc.SENSITIVITY and len(moved) == 5


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_time_step_references_feel_the_geometry(fp32):
    """The CFL sum and the corrected and parity dt of the adaptive cases' first step.  dt_v of the
    parity mode is cfl Re / (1 / dy^2 + (NX / 3 LX)^2 + (NZ / 3 LZ)^2) with 1 / dy^2 = 256 against box
    terms of 1.6 and 2.1: a mutated box moves it by 4e-3 to 2e-2, so its floor is 1e-3, 1000 x the
    1e-6 it is held to (test_dt_update_kernel holds the same formula to 1e-14 on this box)."""
    dt, state = gc.step_state(gc.SMALL, gc.GEOM_A, fp32)
    which = {k: v for k, v in gc.ADAPTIVE_WHICH.items() if k != "dt_v_parity"}
    moved = gc.assert_geometry_sensitive(gc.first_adaptive_step, gc.GEOM_A, state, which, gc.SMALL, **gc.ADAPTIVE)
    assert _report("adaptive dt", moved) >= gc.SENSITIVITY and len(moved) == 4
    moved = gc.assert_geometry_sensitive(gc.first_adaptive_step, gc.GEOM_A, state, {"dt_v_parity": gc.BOX}, gc.SMALL,
                                         floor=1e-3, **gc.ADAPTIVE)
    assert _report("parity dt_v", moved) >= 1e-3 and len(moved) == 3


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_diagnostics_references_feel_the_geometry(fp32):
    """Every diagnostics reference (plane statistics, spectra, gradient sums, triple products, moments,
    Pi, p', pressure moments, p-hat', pressure strain, plane spectra with the pressure row,
    cross-spectra, the rotational term, spectral budgets, the physical fields but omega_y, the wall
    shear) under the three box mutations and the stretch."""
    state = gc.diagnostics_reference(fp32)["state"]
    moved = gc.assert_geometry_sensitive(gc.diagnostics_arrays, gc.GEOM_A, state, gc.BOX_Y, gc.SMALL)
    assert _report("diagnostics", moved) >= gc.SENSITIVITY and len(moved) == 4
    assert all(len(d) == len(gc.DIAG_ARRAYS) + len(gc.PHYS_SENSITIVE) + 2 for d in moved.values())


def test_omega_y_is_the_state():
    """Why omega_y is left out of the preconditions: the prepared field is omega itself."""
    d = gc.diagnostics_reference()
    om = np.array(d["state"][1])
    om[:, 0, 0] = 0
    assert np.array_equal(d["o"].fields[4], om)


def test_ts_wave_on_the_long_box_is_another_wave_without_ax():
    """test_geometry_gpu.py's TS wave at LX = 4 pi, kx index 2 has alpha = 1; a solver that ignored ax
    would advance an alpha = 2 wave, whose Orr-Sommerfeld growth rate is far outside the 1 % band."""
    plan = ora.OraclePlan(16, 129, 9, LX=gc.GEOM_B["LX"])
    assert abs(plan.ax * 2 - 1.0) < 1e-15 and plan.Kx >= 2
    c1 = osm.least_stable(7500.0, 1.0)[0]
    c2 = osm.least_stable(7500.0, 2.0)[0]
    s1, s2 = 1.0 * np.imag(c1), 2.0 * np.imag(c2)
    print(f"growth rates: alpha = 1 {s1:.6e}, alpha = 2 {s2:.6e}")
    assert s1 > 0 and abs(s2 - s1) > 0.5 * s1


def test_wrapper_axes_differ_from_the_default_box():
    a = gc.make_oracle(*gc.SMALL, gc.GEOM_A).plan
    kx, kz = a.ax * np.arange(a.Kx + 1), a.az * np.arange(a.nkz)
    assert gc.change(np.arange(a.Kx + 1.0), kx) >= gc.SENSITIVITY and gc.change(2.0 * np.arange(a.nkz), kz) >= gc.SENSITIVITY


# ---- the oracle on GEOM_A (tolerances of test_oracle_cpu.py) -----------------------------------------
def _oracle_a():
    dt, state = gc.step_state(gc.SMALL, gc.GEOM_A, False)
    o = gc.make_oracle(*gc.SMALL, gc.GEOM_A, dt_fixed=dt)
    o.set_state(*state)
    return o


def test_continuity_of_recovered_velocity():
    o = _oracle_a()
    o.prepare()
    u, v, w = (o.lines(f) for f in o.fields[:3])
    div = 1j * o.al * u + o.ops.D1 @ v + 1j * o.be * w
    assert np.abs(div).max() < 1e-12 * max(1.0, np.abs(v).max())
    # (precondition) with the default box's wavenumbers the same fields are not divergence-free
    d = ora.OracleSolver(*gc.SMALL)
    div = 1j * d.al * u + o.ops.D1 @ v + 1j * d.be * w
    assert np.abs(div).max() > 1e-2 * np.abs(o.ops.D1 @ v).max()


def test_flux_and_wall_conditions_after_steps():
    o = _oracle_a()
    assert abs(o.ops.trap @ o.U - gc.GEOM_A["Q"]) < 1e-12 and abs(gc.GEOM_A["Q"] - 1.8) > 0.1
    for _ in range(gc.NSTEPS):
        o.step()
    vl = ora._bsolve(ora.helm_matrix(o.ops, o.k2), o.ops.M @ o.lines(o.phi))
    dv = o.ops.D1 @ vl
    nz = o.k2 > 0
    assert np.abs(vl[[0, -1]]).max() < 1e-12
    assert np.abs(dv[[0, -1]][:, nz]).max() < 1e-11
    assert abs(o.ops.trap @ o.U - gc.GEOM_A["Q"]) < 1e-12


# ---- the statistics rebuild their operators from the stretch --------------------------------------------
def test_statistics_take_the_stretch():
    n = gc.SMALL[1]
    ops = ora.build_ops(n, gc.GEOM_A["stretch"])
    assert np.abs(ops.y - ora.build_ops(n).y).max() > 1e-2
    st = TurbulenceStatistics(ops.y, 1.0 / gc.RE, stretch=gc.GEOM_A["stretch"])
    assert np.array_equal(st._ops().D1, ops.D1)
    pm = np.zeros((4, n))
    pm[2] = 1 - ops.y ** 2
    st.add_pressure(pm)
    assert np.abs(st.pressure_terms()["pdiff_k"] - 2 * ops.y).max() < 1e-3
    bad = TurbulenceStatistics(ops.y, 1.0 / gc.RE)
    bad.add_pressure(pm)
    with pytest.raises(ValueError, match="not the tanh grid of this stretch"):
        bad.pressure_terms()
