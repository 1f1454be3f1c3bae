"""The passive scalar on the GPU (zscalar_kernel, scalar_kernel, their place in the step graph and the state
operations) against the NumPy reference (reference/scalar.py) on the same state: random_state(seed=3,
amp=0.3), a random theta of amplitude 0.2 with the mean line y, walls -+1, Re = 400, Pr = 0.71.

Tolerances: the flux pass relative to max |F|, 1e-9 in fp64 and 1e-5 in fp32 (those of
test_pressure_gpu.py); whole steps at relative L2 < 1e-9 in fp64 (test_gpu_matches_oracle_fp64) and, in
fp32, omega_y's 1e-4 max(1, NY / 600) of test_gpu_matches_oracle_large_ny: theta obeys omega_y's equation.
fp32 storage: the oracle is given the complex64-rounded state, so the rounding of the state is shared."""
import functools
import math

import numpy as np
import pytest

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import scalar as sca
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE, PR = 400.0, 0.71
BOX = dict(LX=8 * math.pi / 3, LZ=5 * math.pi / 4, stretch=1.6)  # the box of tests/test_geometry_gpu.py


def _round32(a):
    return a.astype(np.complex64).astype(complex)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _oracle(NX, NY, NZ, fp32, dt, box=()):
    o = sca.ScalarOracle(NX=NX, NY=NY, NZ=NZ, Re=RE, dt_fixed=dt, Pr=PR, wall=(-1.0, 1.0), **dict(box))
    phi, om = ora.random_state(o.plan, o.ops, seed=3, amp=0.3)
    th = sca.random_scalar(o.plan, o.ops, seed=4, amp=0.2, mean=o.ops.y)
    if fp32:
        phi, om, th = _round32(phi), _round32(om), _round32(th)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.set_scalar(th)
    return o


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32, dt=0.01, box=(), steps=0):
    """The state, the fluxes of the initial state and theta after each of `steps` steps; computed once per
    case, read-only."""
    o = _oracle(NX, NY, NZ, fp32, dt, box)
    d = dict(phi=o.phi.copy(), om=o.om.copy(), U=o.U.copy(), th=o.th.copy())
    o.prepare()
    d["F"] = o.scalar_flux()
    d["sums"] = sca.scalar_sums(o)
    d["steps"] = []
    for _ in range(steps):
        o.step()
        d["steps"].append(o.th.copy())
    for a in [d["phi"], d["om"], d["U"], d["th"], d["F"], d["sums"]] + d["steps"]:
        a.setflags(write=False)
    return d


def _config(NX, NY, NZ, precision, dt=0.01, **kw):
    return default_config(**{**dict(NX=NX, NY=NY, NZ=NZ, Re=RE, precision=precision, ic="zero", log_every=0, symmetry_every=0,
                                    stats_every=0, dt_fixed=dt, scalar=True, Pr=PR, scalar_lower=-1.0, scalar_upper=1.0,
                                    scalar_ic="zero"), **kw})


def _solver(native, NX, NY, NZ, precision, dt=0.01, box=(), steps=0, **kw):
    s = native.Solver(_config(NX, NY, NZ, precision, dt, **dict(box), **kw), 0, 1, 0, b"")
    ref = _reference(NX, NY, NZ, precision == "fp32", dt, tuple(box), steps)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.set_scalar(ref["th"])
    s.prepare()
    return s, ref


# ---- 1. the flux pass alone -----------------------------------------------------------------------------
def _check_flux(s, ref, precision, what):
    got = s.scalar_flux_hat()
    want = ref["F"]
    assert got.shape == want.shape and got.dtype == np.complex128 and np.isfinite(got).all()
    tol = 1e-9 if precision == "fp64" else 1e-5
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: flux rel. error {err:.3e} (tol {tol:.1e})")
    assert err < tol
    return got


@pytest.mark.parametrize("NX,NY,NZ,precision", [(32, 33, 17, "fp64"), (32, 33, 17, "fp32"), (48, 33, 41, "fp64"),
                                                (48, 33, 41, "fp32"), (16, 17, 513, "fp32"), (16, 17, 513, "fp64"),
                                                (16, 17, 1025, "fp32")])
def test_flux_pass(native, NX, NY, NZ, precision):
    """Packed rows (32 points), radix-3 and radix-5 lengths (48, 80), 1024-point rows on one wave (fp32) or
    two (fp64), 2048 points on two waves."""
    s, ref = _solver(native, NX, NY, NZ, precision)
    got = _check_flux(s, ref, precision, f"{NX}x{NY}x{NZ} {precision}")
    # kz = 0 plane Hermitian: the kz = 0 imaginary parts of the inputs are dropped
    p = s.plan
    i = np.arange(1, p.Kx + 1)
    herm = np.abs(got[:, :, p.nkx - i, 0] - np.conj(got[:, :, i, 0])).max() / np.abs(got).max()
    print(f"kz = 0 Hermitian defect of the fluxes {herm:.2e}")
    assert herm <= (1e-12 if precision == "fp64" else 1e-5)
    assert np.array_equal(got, s.scalar_flux_hat())  # repeatable: the state is not written


def test_flux_pass_partial_last_chunk(native, monkeypatch):
    s, ref = _solver(native, 32, 33, 17, "fp64")
    whole = _check_flux(s, ref, "fp64", "32x33x17 fp64 unchunked")
    monkeypatch.setenv("CHANNEL_YCHUNK", "8")
    s2, _ = _solver(native, 32, 33, 17, "fp64")
    assert np.array_equal(s2.scalar_flux_hat(), whole)


def test_flux_pass_blocked_layout(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check_flux(s, ref, "fp64", "32x33x17 fp64 blocked")


def test_flux_pass_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check_flux(s, ref, "fp64", "32x33x17 fp64 combine")


# ---- 2. whole steps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("NX,NY,NZ,box", [(32, 33, 17, ()), (48, 33, 41, ()), (32, 33, 17, tuple(BOX.items()))])
def test_steps_match_oracle_fp64(native, NX, NY, NZ, box):
    dt = 0.01 * min(1.0, 32.0 / NX)
    s, ref = _solver(native, NX, NY, NZ, "fp64", dt, box, steps=3)
    for it in range(3):
        s.step(False)
        e = rel(s.get_scalar(), ref["steps"][it])
        print(f"{NX}x{NY}x{NZ} step {it}: theta rel. L2 {e:.3e}")
        assert e < 1e-9, f"theta step {it}"


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("NY", [129, 385, 633])
def test_steps_match_oracle_tall_lines(native, NY, precision):
    """R = 3, 7 (the blocked layout by default) and 10 (which spills in fp64)."""
    NX, NZ, dt = 16, 9, 1e-4
    s, ref = _solver(native, NX, NY, NZ, precision, dt, steps=2)
    tol = 1e-9 if precision == "fp64" else 1e-4 * max(1.0, NY / 600)
    for it in range(2):
        s.step(False)
        e = rel(s.get_scalar(), ref["steps"][it])
        print(f"NY = {NY} {precision} step {it}: theta rel. L2 {e:.3e} (tol {tol:.1e})")
        assert e < tol, f"theta step {it}: {e:.3e}"


# ---- 3. passivity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_scalar_is_passive(native, precision):
    s, ref = _solver(native, 32, 33, 17, precision)
    b = native.Solver(_config(32, 33, 17, precision, scalar=False, scalar_lower=0.0, scalar_upper=0.0, scalar_ic="laminar"), 0, 1, 0, b"")
    b.set_state(ref["phi"], ref["om"], ref["U"])
    b.prepare()
    for _ in range(3):
        s.step(False)
        b.step(False)
    for x, y in zip(s.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    assert rel(s.get_scalar(), ref["th"]) > 1e-3  # (theta did move)
    with pytest.raises(RuntimeError, match="scalar"):
        b.get_scalar()


# ---- 4. exact states ------------------------------------------------------------------------------------
def _laminar_solver(native, **kw):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="laminar", log_every=0, symmetry_every=0, stats_every=0,
                         dt_fixed=0.01, scalar=True, Pr=PR, **kw)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    return s


def test_conduction_profile_is_steady(native):
    s = _laminar_solver(native, scalar_lower=-1.0, scalar_upper=1.0)
    y = np.asarray(s.grid.y)
    th = s.get_scalar()
    assert np.abs(th[:, 0, 0] - y).max() < 1e-15  # scalar_ic = "laminar"
    for _ in range(20):
        s.step(False)
    th = s.get_scalar()
    drift = np.abs(th[:, 0, 0] - y).max()
    print(f"conduction drift after 20 steps {drift:.2e}")
    assert drift < 1e-12
    th[:, 0, 0] = 0
    assert np.abs(th).max() == 0.0


def test_internal_heating_profile_is_steady(native):
    S = 0.3
    s = _laminar_solver(native, scalar_source=S)
    y = np.asarray(s.grid.y)
    want = S * (1 - y * y) * RE * PR / 2
    th = s.get_scalar()
    assert np.abs(th[:, 0, 0] - want).max() < 1e-13 * want.max()  # scalar_ic = "laminar"
    for _ in range(20):
        s.step(False)
    drift = np.abs(s.get_scalar()[:, 0, 0] - want).max() / want.max()
    print(f"heating relative drift after 20 steps {drift:.2e}")
    assert drift < 1e-12


# ---- 5. the linear rate, independent of the oracle --------------------------------------------------------
def test_linear_rate_matches_eigenvalue(native):
    """One mode (kx, kz) = (1, 1) on the laminar U: the measured rate against the least-damped eigenvalue of
    kappa (D2 - k2) - i al U, within the NumPy reference's own deviation plus 1e-9 / (50 dt) = 1e-8, what a
    1e-9 agreement per step permits over the run."""
    dt, n = 0.002, 50
    lam, v = sca.linear_rate(NY=33, Re=RE, Pr=PR)

    def rate(step, get):
        a0 = np.vdot(v, get())
        for _ in range(n):
            step()
        return np.log(np.vdot(v, get()) / a0) / (n * dt)

    o = sca.ScalarOracle(NX=32, NY=33, NZ=17, Re=RE, dt_fixed=dt, Pr=PR)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(np.zeros_like(o.phi), np.zeros_like(o.om), U)
    th = np.zeros_like(o.th)
    th[:, 1, 1] = 1e-3 * v
    o.set_scalar(th)
    own = abs(rate(o.step, lambda: o.th[:, 1, 1]) - lam)
    s = native.Solver(_config(32, 33, 17, "fp64", dt, scalar_lower=0.0, scalar_upper=0.0), 0, 1, 0, b"")
    s.set_state(np.zeros_like(o.phi), np.zeros_like(o.om), U)
    s.set_scalar(th)
    s.prepare()
    r = rate(lambda: s.step(False), lambda: s.get_scalar()[:, 1, 1])
    print(f"device rate {r:.11f}, eigenvalue {lam:.11f}: deviation {abs(r - lam):.3e}; the reference's own {own:.3e}")
    assert abs(r - lam) <= own + 1e-8


# ---- 6. plumbing ------------------------------------------------------------------------------------------
def _run5(native, **kw):
    s, _ = _solver(native, 32, 33, 17, "fp32", **kw)
    return s


def test_graph_replay_equals_eager(native):
    a, b = _run5(native), _run5(native)
    b.set_use_graph(False)
    for _ in range(5):
        a.step(False)
        b.step(False)
    assert a.graph_active() and not b.graph_active()
    assert np.array_equal(a.get_scalar(), b.get_scalar())
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)


def test_lds_poison_is_bitwise(native):
    a = _run5(native)
    for _ in range(2):
        a.step(False)
    fa = a.scalar_flux_hat()
    native.set_lds_poison(True)
    try:
        b = _run5(native)
        for _ in range(2):
            b.step(False)
        fb = b.scalar_flux_hat()
        th_b = b.get_scalar()
    finally:
        native.set_lds_poison(False)
    assert np.array_equal(a.get_scalar(), th_b) and np.array_equal(fa, fb)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_restart_round_trip(native, tmp_path, precision):
    """theta read back from output.T is bitwise the theta written in fp64 (the file's units NX Nzp are a power
    of two here) and within float32 rounding in fp32."""
    if not native.hdf5_available():
        pytest.skip("hdf5 missing")
    g, d, t = (str(tmp_path / n) for n in ("G.h5", "DDV.h5", "T.h5"))
    a, _ = _solver(native, 32, 33, 17, precision)
    for _ in range(2):
        a.step(False)
    a.write_restart(g, d, "-", t)
    th_a = a.get_scalar()
    b = native.Solver(_config(32, 33, 17, precision, ic="file", in_G=g, in_DDV=d, in_T=t, scalar_ic="file"), 0, 1, 0, b"")
    b.read_restart(g, d, "-", t)
    b.prepare()
    if precision == "fp64":
        assert np.array_equal(b.get_scalar(), th_a)
    else:  # through the file's float32 and its units (NX Nzp)
        assert rel(b.get_scalar(), th_a) < 1e-6
    for x, y in zip(a.get_state(), b.get_state()):
        assert rel(x, y) < (1e-15 if precision == "fp64" else 1e-6)
    # one more step: bitwise that of a solver handed the same state in memory; the run that wrote the files
    # goes on from K-SPEC's outputs of its last substep, not from prepare()'s, so it agrees to rounding only
    c, _ = _solver(native, 32, 33, 17, precision)
    c.set_state(*a.get_state())
    c.set_scalar(th_a)
    c.prepare()
    for s_ in (a, b, c):
        s_.step(False)
    if precision == "fp64":
        assert np.array_equal(b.get_scalar(), c.get_scalar())
        assert rel(b.get_scalar(), a.get_scalar()) < 1e-13
    # a theta file on another grid is refused, as G is
    other = native.Solver(_config(48, 33, 17, precision, in_T=t, scalar_ic="file"), 0, 1, 0, b"")
    with pytest.raises(RuntimeError, match="input.T must be on the solver's grid"):
        other.init_scalar_ic()


def test_rollback_restores_theta(native):
    s, _ = _solver(native, 32, 33, 17, "fp64")
    s.step(False)
    s.take_snapshot()
    th1 = s.get_scalar()
    s.step(False)
    after = s.get_scalar()
    assert not np.array_equal(after, th1)
    s.rollback()
    assert np.array_equal(s.get_scalar(), th1)
    # (R_theta is cleared like R_phi: the redone step starts at a substep 0, where zeta = 0)
    s.step(False)
    assert rel(s.get_scalar(), after) < 1e-12


def test_symmetrize_repairs_kz0(native):
    s, ref = _solver(native, 32, 33, 17, "fp64")
    s.symmetrize()
    assert np.array_equal(s.get_scalar(), ref["th"])  # a Hermitian theta is unchanged
    bad = ref["th"].copy()
    bad[5, 3, 0] += 0.1 + 0.2j
    s.set_scalar(bad)
    s.symmetrize()
    got = s.get_scalar()
    p = s.plan
    i = np.arange(1, p.Kx + 1)
    assert np.abs(got[:, p.nkx - i, 0] - np.conj(got[:, i, 0])).max() == 0.0
    assert np.array_equal(got[:, :, 1:], bad[:, :, 1:])
    assert np.array_equal(got[:, 0, 0], ref["th"][:, 0, 0])  # the mean profile stays


def test_nan_in_theta_raises_health(native):
    s, ref = _solver(native, 32, 33, 17, "fp32")
    s.step(False)
    assert s.health() == 0
    bad = ref["th"].copy()
    bad[16, 2, 3] = np.nan
    s.set_scalar(bad)
    s.step(False)
    assert s.health() & 1


def test_communicator_is_refused(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    with pytest.raises(RuntimeError, match="scalar = true"):
        ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", stats_every=0, log_every=0, scalar=True)


def test_two_wave_lines_are_refused(native, monkeypatch):
    """CHANNEL_KSPEC_HALVES=1 (fp32, 258 < NY <= 512): refused at construction, not at the first step."""
    monkeypatch.setenv("CHANNEL_KSPEC_HALVES", "1")
    with pytest.raises(RuntimeError, match="scalar = true.*CHANNEL_KSPEC_HALVES"):
        native.Solver(_config(16, 385, 9, "fp32"), 0, 1, 0, b"")
    native.Solver(_config(16, 385, 9, "fp32", scalar=False, scalar_lower=0.0, scalar_upper=0.0), 0, 1, 0, b"")


# ---- 7. scalar_sums ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kzb", ["0", "1"])
def test_scalar_sums(native, monkeypatch, kzb):
    monkeypatch.setenv("CHANNEL_SPEC_KZB", kzb)
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == (8 if kzb == "1" else 0)
    m = s.scalar_sums()
    assert m.shape == (5, 33) and m.dtype == np.float64
    assert np.array_equal(m[0], ref["sums"][0])
    for r in range(1, 5):
        err = np.abs(m[r] - ref["sums"][r]).max() / np.abs(ref["sums"][r]).max()
        print(f"scalar sum row {r}: rel. error {err:.3e}")
        assert err < 1e-12
    assert np.abs(s.scalar_sums() - m).max() <= 1e-14 * np.abs(m).max()  # accumulators are reset per call


def test_scalar_files_and_model(native, tmp_path):
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0, log_every=0,
                    symmetry_every=0, path=str(tmp_path) + "/", scalar=True, Pr=PR, scalar_lower=-1.0, scalar_upper=1.0,
                    scalar_every=2)
    c.initialize()
    assert np.abs(c.get_scalar()[:, 0, 0] - c.y).max() < 1e-6
    th = c.get_scalar()
    th[:, 1, 1] = 0.05 * (1 - c.y ** 2)
    c.set_scalar(th)
    c.run(4, False)
    m = c.scalar_sums()
    want = {"TMEAN": m[0], "TRMS": np.sqrt(m[1]), "UT": m[2], "VT": m[3]}
    for name, now in want.items():
        rows = np.loadtxt(tmp_path / f"{name}.dat")
        assert rows.shape == (2, 33) and np.isfinite(rows).all(), name
        assert np.abs(rows[1] - now).max() <= 2e-8 * np.abs(now).max() + 1e-300, name
    tw = np.loadtxt(tmp_path / "TWALL.dat")
    assert tw.shape == (2, 4) and list(tw[:, 0]) == [2.0, 4.0]
    # the host's compact D1 of Theta against the NumPy one (ten significant digits in the file)
    d = ora.build_ops(33).D1 @ m[0]
    assert np.abs(tw[1, 2:] - d[[0, -1]]).max() <= 1e-9 * np.abs(d[[0, -1]]).max()
    assert tw[1, 1] == pytest.approx(c.log().time, rel=1e-9)


def test_python_driver_writes_theta(native, tmp_path):
    """python -m channel_gpu_amd.driver with output.T: the theta file is written beside G and DDV and a
    second run resumes from it through input.T."""
    import os
    import subprocess
    import sys

    if not native.hdf5_available():
        pytest.skip("hdf5 missing")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = """application:
{{
  NX = 32; NY = 33; NZ = 17;
  input: {{ G = "{gin}"; DDV = "{din}"; UMEAN = "-"; T = "{tin}"; }};
  output: {{ G = "{d}/G.h5"; DDV = "{d}/DDV.h5"; UMEAN = "-"; T = "{d}/T.h5"; }};
  path = "{d}/";
  Re = 400.0; nsteps = {n}; stats_every = 0; log_every = 0; precision = "fp64"; dt_fixed = 0.01;
  ic = "{ic}"; ic_amplitude = 0.3;
  scalar = true; Pr = 0.71; scalar_lower = -1.0; scalar_upper = 1.0;
}};
"""
    da, db = str(tmp_path / "a"), str(tmp_path / "b")
    for d, kw in ((da, dict(gin="-", din="-", tin="-", ic="random", n=2)),
                  (db, dict(gin=f"{da}/G.h5", din=f"{da}/DDV.h5", tin=f"{da}/T.h5", ic="file", n=0))):
        os.makedirs(d)
        with open(os.path.join(d, "run.conf"), "w") as f:
            f.write(conf.format(d=d, **kw))
        r = subprocess.run([sys.executable, "-m", "channel_gpu_amd.driver", os.path.join(d, "run.conf"), "--quiet"],
                           capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr
        assert os.path.exists(os.path.join(d, "T.h5"))
    ta, dims = native.h5_read_planes(os.path.join(da, "T.h5"), list(range(32)))
    tb, _ = native.h5_read_planes(os.path.join(db, "T.h5"), list(range(32)))
    ta = np.asarray(ta)
    assert list(dims) == [32, 33, 34] and np.isfinite(ta).all()
    # plane kx = 0, kz = 0: Theta(y) in the file's units NX Nzp; its wall values are the Dirichlet ones
    th0 = ta.reshape(32, 17, 33, 2)[0, 0, :, 0] / (32 * 32)
    assert th0[0] == -1.0 and th0[-1] == 1.0 and np.abs(np.diff(th0)).max() < 0.3
    assert np.array_equal(ta, np.asarray(tb))  # read through input.T and written again without a step
