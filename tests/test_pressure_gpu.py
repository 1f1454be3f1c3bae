"""Pressure on the GPU (Solver.pressure_hat: the y-line Poisson kernel behind the step's transform
stage; Solver.pressure_moments and physical_fields("p"): the export stage's pressure mode) against the
NumPy reference (reference/pressure.py) on the oracle's fields.

fp32 storage: the oracle is given the complex64-rounded phi and omega, so the rounding of the state is
shared.  Tolerances are the project's own, relative to the maximum of the compared quantity: 1e-9 in
fp64 (the oracle-agreement tolerance of test_combine_mode_matches_oracle), 1e-5 in fp32.  Every fp32
case prints the emulation error beside its result: the reference evaluated from complex64-rounded
fields and H (5.9e-8 to 1.2e-7 of max |Pi| over the shapes here; the device is within 1.3e-7 at R = 1,
2.6e-6 at R = 7 and 7.2e-6 at R = 10: its H also passes the transform stage's fp32 arithmetic)."""
import copy
import functools

import numpy as np
import pytest

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0


def _round32(a):
    return a.astype(np.complex64).astype(complex)


class _Rounded(ora.OracleSolver):
    """The fp32-storage emulation: the prepared fields and H rounded to complex64."""

    def transforms(self, compute_dt):
        super().transforms(compute_dt)
        self.H = _round32(self.H)


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32):
    """Oracle state (complex64-rounded for fp32 storage), its Pi [NY, nkx, nkz], p' [NY, NX, Nzp] and
    pressure moments [4, NY]; computed once per case, read-only.  Also the fp32 emulation error of Pi
    relative to max |Pi|."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    if fp32:
        phi, om = _round32(phi), _round32(om)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    Pi = prs.pressure_hat(o)
    pp = prs.pressure_physical(o, Pi)
    pm = prs.pressure_moments(o, Pi)
    o32 = copy.copy(o)
    o32.__class__ = _Rounded
    o32.fields = _round32(o.fields)
    emu = np.abs(prs.pressure_hat(o32) - Pi).max() / np.abs(Pi).max()
    uph = ora.spec_to_phys_full(o.fields[0], o.plan)
    Pi = Pi.reshape(o.phi.shape)
    for a in (phi, om, U, Pi, pp, pm, uph):
        a.setflags(write=False)
    return dict(phi=phi, om=om, U=U, Pi=Pi, pp=pp, pm=pm, u=uph, emu=float(emu), o=o)


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


def _check_pi(s, ref, precision, what):
    got = s.pressure_hat()
    want = ref["Pi"]
    assert got.shape == want.shape and got.dtype == np.complex128 and np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: Pi rel. error {err:.3e} (tol {_tol(precision):.1e}; fp32 emulation error {ref['emu']:.1e})")
    # the mean line is exactly zero (padding rows and lines of the device layout: pressure_hat itself
    # refuses a non-zero one)
    assert np.array_equal(got[:, 0, 0], np.zeros(got.shape[0], complex))
    assert err < _tol(precision), f"{what}: {err:.3e} >= {_tol(precision):.1e}"
    return got


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_pressure_hat_plain_layout(native, NX, precision):
    """R = 1, the plain layout, a non-power-of-two x length; lines = nkx * nkz is odd: a partial last tile."""
    s, ref = _solver(native, NX, 33, 17, precision)
    assert s.spec_kzb() == 0
    _check_pi(s, ref, precision, f"{NX}x33x17 {precision}")


def test_pressure_hat_tiled_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 rows pad to 40."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check_pi(s, ref, "fp64", "32x33x17 fp64 blocked")


def test_pressure_hat_r3(native):
    s, ref = _solver(native, 16, 129, 9, "fp64")
    _check_pi(s, ref, "fp64", "16x129x9 fp64 (R = 3)")


def test_pressure_hat_r7_natural_tiled(native):
    s, ref = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    _check_pi(s, ref, "fp32", "16x385x9 fp32 (R = 7)")


def test_pressure_hat_r10(native):
    s, ref = _solver(native, 16, 577, 9, "fp32")
    _check_pi(s, ref, "fp32", "16x577x9 fp32 (R = 10)")


def test_pressure_hat_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check_pi(s, ref, "fp64", "32x33x17 fp64 combine")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [48, 32])
def test_physical_pressure_planes(native, NX, precision):
    """NX = 48 rows per plane against 128-row blocks: the blocks straddle planes."""
    s, ref = _solver(native, NX, 33, 17, precision)
    planes = [0, 5, 32]
    f = s.physical_fields(planes, ["p", "u"])
    # "u" is unchanged by asking for "p": bitwise the u of a request that transforms the same (u, v)
    # pair; a request for u alone transforms (u, 0), whose rounding differs (eps of the storage type)
    assert np.array_equal(f["u"], s.physical_fields(planes, ["u", "v"])["u"])
    only_u = s.physical_fields(planes, ["u"])["u"]
    assert np.abs(f["u"] - only_u).max() <= (1e-13 if precision == "fp64" else 1e-6) * np.abs(only_u).max()
    want = ref["pp"][planes]
    p = f["p"]
    assert p.shape == want.shape
    scale = np.abs(ref["pp"]).max()
    err = np.abs(p - want).max() / scale
    print(f"p' planes: rel. error {err:.3e} (tol {_tol(precision):.1e}; fp32 emulation error of Pi {ref['emu']:.1e})")
    assert err < _tol(precision)
    assert np.abs(p.mean(axis=(1, 2))).max() < 1e-12 * scale
    # with a vorticity field beside it (a second export pass), in the request's order
    g = s.physical_fields(planes, ["wz", "p", "v"])
    assert list(g) == ["wz", "p", "v"]
    assert np.array_equal(g["p"], p)
    assert np.array_equal(g["wz"], s.physical_fields(planes, ["wz"])["wz"])
    assert np.array_equal(g["v"], s.physical_fields(planes, ["v"])["v"])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [48, 32])
def test_pressure_moments(native, NX, precision):
    s, ref = _solver(native, NX, 33, 17, precision)
    m = s.pressure_moments()
    assert m.shape == (4, 33) and m.dtype == np.float64 and np.isfinite(m).all()
    for r, n in enumerate(prs.PRESSURE_ROWS):
        err = np.abs(m[r] - ref["pm"][r]).max() / np.abs(ref["pm"][r]).max()
        print(f"pressure moment {n}: rel. error {err:.3e} (tol {_tol(precision):.1e})")
        assert err < _tol(precision), n
    # independently of the reference formulas: row 0 is the plane variance of the exported planes
    p = s.physical_fields(list(range(33)), ["p"])["p"]
    var = (p * p).mean(axis=(1, 2))
    err = np.abs(m[0] - var).max() / var.max()
    print(f"<p'p'> against the variance of the exported planes: rel. error {err:.3e}")
    assert err < _tol(precision)
    # accumulators are reset per call
    assert np.abs(s.pressure_moments() - m).max() <= 1e-12 * np.abs(m).max()


def test_momentum_residual_with_device_pressure(native):
    """The device's Pi in the oracle's momentum equations: the residual is the y-discretisation's error,
    common to the device and the reference; a wrong kernel moves it by O(1)."""
    from channel_gpu_amd.reference import budgets as bud

    dt = 1e-6
    o = ora.OracleSolver(NX=16, NY=129, NZ=9, Re=RE, dt_fixed=dt)
    phi, om = bud.smooth_state(o.plan, o.ops, seed=9, amp=0.3)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    Pi_ref = prs.pressure_hat(o)
    o1 = copy.deepcopy(o)
    o1.step()
    cfg = default_config(NX=16, NY=129, NZ=9, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0, stats_every=0)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.set_state(phi, om, U)
    s.prepare()
    Pi_dev = s.pressure_hat().reshape(129, -1)
    keep = o.k2 > 0
    mx = lambda a: float(np.abs(a[2:-2][:, keep]).max())  # noqa: E731
    r_ref = [mx(r) for r in prs.momentum_residual(o, Pi_ref, o1, dt)]
    r_dev = [mx(r) for r in prs.momentum_residual(o, Pi_dev, o1, dt)]
    for n, a, b in zip("uvw", r_ref, r_dev):
        print(f"{n}-momentum residual: reference Pi {a:.6e}, device Pi {b:.6e}")
        assert abs(b - a) <= 0.01 * a, n


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
    """State, log and mean profile after 4 + 4 steps with the calls in between are bitwise those of 8
    undisturbed steps.  stats() cannot be compared bitwise between two runs, disturbed or not: K-SPEC
    adds each workgroup's plane sums with fp64 atomics in scheduling order (the test prints whether two
    undisturbed runs happen to agree).  It is held bitwise where that is defined, across the calls on
    the same solver (they do not write the accumulators), and between the runs to the reordering bound
    of a sum of n = 21 x 11 line terms: each order is within n eps sum |terms| of the exact sum, so two
    orders differ by at most 2 n eps sum |terms|, with sum |terms| = the row itself for the mean squares
    and <= sqrt(<uu><vv>) for <uv>.  Measured: two undisturbed runs are not bitwise equal either; the
    disturbed run differs by 5.1e-16 of the scale (bound 1.0e-13)."""
    a = _stepping_solver(native, path=str(tmp_path) + "/a_")
    a.run(8, False)
    a2 = _stepping_solver(native, path=str(tmp_path) + "/a2_")
    a2.run(8, False)
    print("stats() of two undisturbed runs bitwise equal:", np.array_equal(np.asarray(a.stats()), np.asarray(a2.stats())))
    b = _stepping_solver(native, path=str(tmp_path) + "/b_")
    b.run(4, False)
    st_before = np.asarray(b.stats()).copy()
    P1 = b.pressure_hat()
    m1 = b.pressure_moments()
    f1 = b.physical_fields([0, 5, 32], ["p"])["p"]
    P2 = b.pressure_hat()
    assert np.array_equal(P1, P2)  # repeatable, bitwise
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
    sa, sb = np.asarray(a.stats()).reshape(4, 33), np.asarray(b.stats()).reshape(4, 33)
    scale = np.stack([sa[0], sa[1], sa[2], np.sqrt(sa[0] * sa[1])])
    d = np.abs(sa - sb)
    print(f"stats(): bitwise equal {np.array_equal(sa, sb)}, max |difference| / scale {np.max(d[scale > 0] / scale[scale > 0]):.2e}")
    assert (d <= 2 * 21 * 11 * np.finfo(float).eps * scale).all()
    assert np.array_equal(np.asarray(a.mean_profile()), np.asarray(b.mean_profile()))


def test_one_rank_communicator_is_refused(native, monkeypatch, tmp_path, capfd):
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="random", ic_amplitude=0.1, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/", pressure_every=2)
    assert c.solver.comm_kind() != "none"
    c.initialize()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.pressure_hat()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.pressure_moments()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.physical_fields([0], ["p"])
    capfd.readouterr()
    c.run(4, False)
    err = capfd.readouterr().err
    assert err.count("pressure_every") == 1 and "skipped" in err
    assert c.log().step == 4
    assert not (tmp_path / "PRMS.dat").exists()


def test_files_and_sampled_profiles(native, tmp_path):
    Re = 1000.0
    cfg = default_config(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", pressure_every=2,
                         fields_every=4, fields_planes="4,16", fields="u,p")
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    m = s.pressure_moments()
    want = {"PRMS": np.sqrt(m[0]), "PU": m[1], "PV": m[2]}
    for name, now in want.items():
        rows = np.loadtxt(tmp_path / f"{name}.dat")
        assert rows.shape == (2, 33) and np.isfinite(rows).all(), name
        # (nine significant digits in the files; the sums are atomics, equal to rounding only)
        assert np.abs(rows[1] - now).max() <= 2e-8 * np.abs(now).max(), name
    now = s.physical_fields([4, 16], ["u", "p"])
    for n in ("u", "p"):
        a = np.load(tmp_path / f"FIELD_{n}_00000004.npy")
        assert a.shape == (2, 32, 32) and a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, now[n].astype(np.float32)), n

    from channel_gpu_amd.models.channel import ChannelFlow
    from channel_gpu_amd.models.statistics import PRESSURE_TERMS

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
    c.initialize()
    p = c.sample_statistics(8, every=2, budgets=True, pressure=True).profiles()
    assert c.statistics.npr == 4
    for k in ["p_rms", "pu", "pv", "closure_k"] + list(PRESSURE_TERMS):
        assert k in p and p[k].shape == (17,) and np.isfinite(p[k]).all(), k
    assert p["p_rms"].max() > 0
