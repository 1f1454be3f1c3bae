"""Physical-space export (Solver.physical_fields: x-backward + the z complex-to-real stage) and the
one-point moments (Solver.plane_moments) against the NumPy oracle's physical fields."""
import functools
import json

import numpy as np
import pytest

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

NAMES = ["u", "v", "w", "wx", "wy", "wz"]


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ):
    """Oracle state and its six physical fields [6, NY, NX, Nzp] (computed once per grid, read-only)."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    ph = ora.spec_to_phys_full(o.fields, o.plan)
    for a in (phi, om, U, ph):
        a.setflags(write=False)
    return phi, om, U, ph


def _solver(native, NX, NY, NZ, precision, **kw):
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision=precision, ic="zero", log_every=0, symmetry_every=0,
                         **{"stats_every": 0, **kw})
    s = native.Solver(cfg, 0, 1, 0, b"")
    phi, om, U, ph = _reference(NX, NY, NZ)
    s.set_state(phi, om, U)
    s.prepare()
    return s, ph, U


def _check(got, ref, tol, what, field=None):
    """Largest error of the requested planes relative to the maximum of the whole field."""
    err = np.abs(got - ref).max() / np.abs(ref if field is None else field).max()
    print(f"{what}: rel. error {err:.3e} (tol {tol:.1e})")
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"


def _tol(precision):
    return 1e-10 if precision == "fp64" else 1e-5


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_all_fields_all_planes(native, precision):
    s, ph, U = _solver(native, 32, 33, 17, precision)
    f = s.physical_fields(list(range(33)), NAMES)
    assert sorted(f) == sorted(NAMES)
    for i, n in enumerate(NAMES):
        assert f[n].shape == (33, 32, 32) and f[n].dtype == np.float64
        _check(f[n], ph[i], _tol(precision), n)
    assert np.abs(f["u"].mean(axis=(1, 2)) - U).max() < _tol(precision) * np.abs(U).max()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_odd_factor_lengths(native, precision):
    """NX = Nzp = 48: radix-3 plans, several rows per wave."""
    s, ph, _ = _solver(native, 48, 33, 25, precision)
    planes = [0, 7, 32]
    f = s.physical_fields(planes, ["u", "v", "w"])
    for i, n in enumerate(["u", "v", "w"]):
        assert f[n].shape == (3, 48, 48)
        _check(f[n], ph[i][planes], _tol(precision), n, ph[i])


def test_blocked_layout_odd_planes(native):
    """The blocked spectral layout (R = 7): single odd planes and a run across an 8-plane tile edge.
    Fields u, w, omega_z (all three transform pairs).  v is left out: at NY = 385 the fp32 rounding of
    the phi state alone, before any export, moves K-SPEC's v by 8.9e-6 of its maximum at plane 191
    (the oracle run on the complex64-rounded state against the unrounded one; u, w, omega_z: below
    4e-7), which would leave the 1e-5 bound no room for the stage under test."""
    s, ph, _ = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    sel = {"u": 0, "w": 2, "wz": 5}
    for y in (1, 191, 384):
        f = s.physical_fields([y], list(sel))
        for n, i in sel.items():
            assert f[n].shape == (1, 16, 16)
            _check(f[n][0], ph[i][y], 1e-5, f"{n} plane {y}", ph[i])
    run = [6, 7, 8, 9]
    f = s.physical_fields(run, list(sel))
    for n, i in sel.items():
        _check(f[n], ph[i][run], 1e-5, f"{n} planes 6..9", ph[i])


def test_plane_tile_kernel_odd_planes(native, monkeypatch):
    """The wide x-backward of the blocked layout (NX = 512 fp32: tiles of two planes x one 8-wide kz
    block), which the step only launches from its chunk starts: single planes, an odd start and odd
    plane counts, the last plane.  The blocked layout is forced so that NY can stay small."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ph, _ = _solver(native, 512, 33, 9, "fp32")
    assert s.spec_kzb() == 8
    for planes in ([1], [32], [6, 7, 8, 9], [7, 8, 9], [15, 16, 17, 18, 19]):
        f = s.physical_fields(planes, ["u", "v", "w"])
        args = native.xfft_last_backward_variant().split("<")[1].rstrip(">").split(", ")
        assert args[0] == "512" and args[3] == "1" and args[6] == "2", args  # wide, plane tiles
        for i, n in enumerate(["u", "v", "w"]):
            _check(f[n], ph[i][planes], 1e-5, f"{n} planes {planes}", ph[i])


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("NZ", [513, 1025])
def test_long_rows(native, NZ, precision):
    """Nzp = 1024 (one wave per row in fp32) and 2048 (two waves per row)."""
    s, ph, _ = _solver(native, 16, 17, NZ, precision)
    planes = [0, 8]
    f = s.physical_fields(planes, ["u", "wz"])
    assert f["u"].shape == (2, 16, 2 * NZ - 2)
    _check(f["u"], ph[0][planes], _tol(precision), "u", ph[0])
    _check(f["wz"], ph[5][planes], _tol(precision), "wz", ph[5])


def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ph, _ = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    f = s.physical_fields(list(range(33)), NAMES)
    for i, n in enumerate(NAMES):
        _check(f[n], ph[i], 1e-9, n)


def _stepping_solver(native):
    dt = 1e-3
    cfg = default_config(NX=32, NY=33, NZ=17, Re=400.0, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=dt)
    s = native.Solver(cfg, 0, 1, 0, b"")
    phi, om, U, _ = _reference(32, 33, 17)
    s.set_state(phi, om, U)
    s.prepare()
    return s, dt


def test_after_graph_replayed_steps(native):
    s, dt = _stepping_solver(native)
    phi, om, U, _ = _reference(32, 33, 17)
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=400.0, dt_fixed=dt)
    o.set_state(phi, om, U)
    for _ in range(4):
        o.step()
        s.step(False)
    assert s.graph_active()
    o.prepare()
    ph = ora.spec_to_phys_full(o.fields, o.plan)
    f = s.physical_fields(list(range(33)), NAMES)
    for i, n in enumerate(NAMES):
        _check(f[n], ph[i], 1e-9, n)


def test_export_does_not_disturb_the_run(native):
    a, _ = _stepping_solver(native)
    for _ in range(4):
        a.step(False)
    b, _ = _stepping_solver(native)
    for _ in range(2):
        b.step(False)
    b.physical_fields(list(range(33)), NAMES)
    b.plane_moments()
    for _ in range(2):
        b.step(False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    assert La.dt == Lb.dt and La.time == Lb.time


def _numpy_moments(ph, U):
    u = ph[0] - U[:, None, None]
    v, w = ph[1], ph[2]
    rows = [u, u * u, v * v, w * w, u * v, u ** 3, v ** 3, w ** 3, u ** 4, v ** 4, w ** 4]
    return np.stack([r.mean(axis=(1, 2)) for r in rows])


def _moment_tolerances(precision, ph, U, ref):
    """Per-row tolerances relative to each row's maximum: 1e-10 in fp64; in fp32 1e-5, and for the
    third and fourth orders 4x the error of the float32-rounded oracle fields' moments where that
    exceeds 2.5e-6 (the factor covers the transform's own fp32 round-off, which the emulation
    leaves out).  Measured emulation errors (rows 5..10 = u'^3 .. w'^4): 48x33x17: 1.5e-8 2.3e-8
    1.6e-8 4.0e-9 1.4e-8 2.0e-9; 32x33x17: 6.3e-9 2.2e-8 2.7e-8 1.9e-9 1.6e-8 1.1e-8 -- all below
    2.5e-6, so every row is held to 1e-5."""
    if precision == "fp64":
        return np.full(11, 1e-10)
    emu = _numpy_moments(ph.astype(np.float32).astype(np.float64), U)
    e = np.abs(emu - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("fp32 emulation error of rows 5..10:", " ".join(f"{x:.1e}" for x in e[5:]))
    tol = np.full(11, 1e-5)
    tol[5:] = np.where(e[5:] > 2.5e-6, 4 * e[5:], 1e-5)
    return tol


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [48, 32])
def test_moments(native, NX, precision):
    """NX = 48 rows per plane against 128-row blocks: the blocks straddle planes."""
    s, ph, U = _solver(native, NX, 33, 17, precision, stats_every=1)
    m = s.plane_moments()
    assert m.shape == (11, 33)
    ref = _numpy_moments(ph[:3], U)
    tol = _moment_tolerances(precision, ph[:3], U, ref)
    for r in range(1, 11):
        err = np.abs(m[r] - ref[r]).max() / np.abs(ref[r]).max()
        print(f"moment row {r}: rel. error {err:.3e} (tol {tol[r]:.1e})")
        assert err < tol[r], f"moment row {r}: {err:.3e} >= {tol[r]:.1e}"
    # (b) the mean of u' against max |U|
    assert np.abs(m[0]).max() <= tol[0] * np.abs(U).max()
    # the physical-space sums against K-SPEC's Parseval sums of the same prepared state
    st = np.asarray(s.stats()).reshape(4, 33)
    for r in range(4):
        err = np.abs(m[1 + r] - st[r]).max() / np.abs(st[r]).max()
        print(f"moment row {1 + r} vs K-SPEC stats: rel. error {err:.3e}")
        assert err < tol[1 + r]


def test_files(native, tmp_path):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/",
                         fields_every=2, fields_planes="4,16", fields="u,wz", moments_every=2)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    now = s.physical_fields([4, 16], ["u", "wz"])
    for n in ("u", "wz"):
        for step in (2, 4):
            a = np.load(tmp_path / f"FIELD_{n}_{step:08d}.npy")
            assert a.shape == (2, 32, 32) and a.dtype == np.float32
            assert np.isfinite(a).all()
        assert np.array_equal(a, now[n].astype(np.float32))
    side = json.loads((tmp_path / "FIELDS_00000004.json").read_text())
    assert side["planes"] == [4, 16] and side["step"] == 4 and side["NX"] == 32 and side["Nzp"] == 32
    assert len(side["y"]) == 2 and side["time"] > 0 and side["LX"] > 0 and side["LZ"] > 0
    for q in "UVW":
        for kind in ("SKEW", "FLAT"):
            rows = np.loadtxt(tmp_path / f"{q}{kind}.dat")
            assert rows.shape == (2, 33) and np.isfinite(rows).all()


def test_refusals(native, monkeypatch):
    s, _, _ = _solver(native, 32, 33, 17, "fp32")
    with pytest.raises(RuntimeError, match="unknown field"):
        s.physical_fields([0], ["q"])
    with pytest.raises(RuntimeError, match="plane 33"):
        s.physical_fields([33], ["u"])
    # a one-rank communicator (the P > 1 pipeline): the export is refused
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=400.0, precision="fp32", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0)
    assert c.solver.comm_kind() != "none"
    with pytest.raises(RuntimeError, match="single-rank"):
        c.physical_fields([0], ["u"])
    with pytest.raises(RuntimeError, match="single-rank"):
        c.plane_moments()
