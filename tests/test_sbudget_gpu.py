"""Spectral Reynolds-stress budgets at every plane on the GPU (Solver.spectral_budgets: the sbudget
kernel in its two stages) against the NumPy reference (reference/spectral_budgets.py) on the oracle's
fields, against what the solver already has (gradient_sums(), pressure_strain(), physical_fields()) and
against the evolution of the plane spectra over two steps.

Tolerances as tests/test_yspectra_gpu.py, relative to the maximum of a row over all (y, k): 1e-10 in
fp64, 1e-5 in fp32 storage (the oracle is given the complex64-rounded phi and omega), 1e-9 in the
combine mode, 1e-12 between two device results (the atomics are unordered)."""
import functools
import json

import numpy as np
import pytest

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.reference import spectral_budgets as sbr
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0
ROWS = sbr.SBUDGET_ROWS


def _round32(a):
    return a.astype(np.complex64).astype(complex)


def _state(NX, NY, NZ, fp32=False):
    plan, ops = ora.OraclePlan(NX, NY, NZ), ora.build_ops(NY)
    phi, om = ora.random_state(plan, ops, seed=9, amp=0.3)
    if fp32:
        phi, om = _round32(phi), _round32(om)
    return phi, om, 0.75 * 1.8 * (1 - ops.y ** 2)


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32):
    """Oracle state (complex64-rounded for fp32 storage), the prepared oracle, its rotational term and
    its budget rows; computed once per case, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om, U = _state(NX, NY, NZ, fp32)
    o.set_state(phi, om, U)
    o.prepare()
    H = prs.rotational_hat(o)
    sb = sbr.spectral_budgets(o, H=H)
    H = H.reshape((3,) + o.phi.shape)
    for a in (phi, om, U, H, sb["ekx"], sb["ekz"]):
        a.setflags(write=False)
    return dict(o=o, phi=phi, om=om, U=U, H=H, ekx=sb["ekx"], ekz=sb["ekz"])


def _solver(native, NX, NY, NZ, precision, **kw):
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=RE, precision=precision, ic="zero", log_every=0, symmetry_every=0,
                         **{"stats_every": 0, **kw})
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(NX, NY, NZ, precision == "fp32")
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s, ref


def _tol(precision):
    return 1e-10 if precision == "fp64" else 1e-5


def _check_row(got, ref, tol, what, scale=None):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale)
    print(f"{what}: rel. error {err:.3e} (tol {tol:.1e})")
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"


def _check(sb, ref, tol, what):
    """All rows of a spectral_budgets() result against ref["ekx"], ref["ekz"]; every row is reported
    before the first failure is raised."""
    assert list(sb["rows"]) == list(ROWS)
    bad = []
    for e in ("ekx", "ekz"):
        assert sb[e].dtype == np.float64 and sb[e].shape == ref[e].shape, e
        for r in range(20):
            try:
                _check_row(sb[e][r], ref[e][r], tol, f"{what} {e} row {ROWS[r]}")
            except AssertionError as x:
                bad.append(str(x))
    assert not bad, "; ".join(bad)


def _check_inputs(s, ref, tol, what):
    H = s.rotational_hat()
    assert H.shape == ref["H"].shape and H.dtype == np.complex128
    for c in range(3):
        _check_row(H[c], ref["H"][c], tol, f"{what} rotational_hat component {c}")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_plain_layout(native, NX, precision):
    s, ref = _solver(native, NX, 33, 17, precision)
    assert s.spec_kzb() == 0
    sb = s.spectral_budgets()
    p = s.plan
    assert sb["ekx"].shape == (20, 33, p.Kx + 1) and sb["ekz"].shape == (20, 33, p.nkz)
    # (the mean profile as the solver holds it, rounded in fp32 storage, and the compact D1 of that)
    assert np.abs(sb["U"] - ref["U"]).max() < _tol(precision) and np.abs(sb["dU"] - ref["o"].ops.D1 @ sb["U"]).max() < 1e-12
    _check_inputs(s, ref, _tol(precision), "plain")
    _check(sb, ref, _tol(precision), "plain")
    # accumulators are reset per call
    _check(s.spectral_budgets(), ref, _tol(precision), "plain (second call)")


def test_blocked_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 planes pad to 40: a kernel that reads the padding or drops the
    last partial tile shows."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check_inputs(s, ref, 1e-10, "blocked")
    _check(s.spectral_budgets(), ref, 1e-10, "blocked")
    _check(s.spectral_budgets(), ref, 1e-10, "blocked (second call)")


def test_blocked_layout_kz_slices(native, monkeypatch):
    """nkz = 86 pads to 88 lines: two 64-line kz slices, the second partial, in fp32 (two elements per
    lane); the 21 kx rows are three kx slices, the middle one with +kx and -kx of the same bins."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 129, "fp32")
    assert s.spec_kzb() == 8 and s.plan.nkz == 86
    _check_inputs(s, ref, 1e-5, "blocked, two kz slices")
    _check(s.spectral_budgets(), ref, 1e-5, "blocked, two kz slices")


def test_blocked_layout_natural(native):
    """R = 7: the blocked layout as the headline grid has it, fp32; plane 384 is alone in its chunk."""
    s, ref = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    _check_inputs(s, ref, 1e-5, "blocked, R = 7")
    _check(s.spectral_budgets(), ref, 1e-5, "blocked, R = 7")


def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check_inputs(s, ref, 1e-9, "combine")
    _check(s.spectral_budgets(), ref, 1e-9, "combine")


def test_against_existing_outputs(native):
    """Independent of the new reference: the k-sums of the g rows are gradient_sums(), those of the
    pressure rows pressure_strain()."""
    s, _ = _solver(native, 32, 33, 17, "fp64")
    sb = s.spectral_budgets()
    g = s.gradient_sums()
    ps = s.pressure_strain()
    for e in ("ekx", "ekz"):
        for q in range(4):
            _check_row(sb[e][4 + q].sum(axis=-1), g[3 + q], 1e-12, f"{e} row {ROWS[4 + q]} summed against gradient_sums()")
        for q in range(6):
            _check_row(sb[e][14 + q].sum(axis=-1), ps[q], 1e-12, f"{e} row {ROWS[14 + q]} summed against pressure_strain()")


def test_against_physical_space(native):
    """u' x omega' formed in NumPy from the exported planes of u, v, w, wx, wy, wz: the plane means of
    u' (u' x omega')_x, v (.)_y, w (.)_z are the k-sums of rows n_uu, n_vv, n_ww."""
    s, ref = _solver(native, 32, 33, 17, "fp64")
    sb = s.spectral_budgets()
    names = ["u", "v", "w", "wx", "wy", "wz"]
    pf = s.physical_fields(list(range(33)), names)
    f = np.stack([np.asarray(pf[n]) for n in names])
    f[0] -= ref["U"][:, None, None]
    f[5] += (ref["o"].ops.D1 @ ref["U"])[:, None, None]  # omega_z' = omega_z + U'
    h = ora.rotational_product(f)
    for c in range(3):
        want = (f[c] * h[c]).mean(axis=(1, 2))
        for e in ("ekx", "ekz"):
            _check_row(sb[e][c].sum(axis=-1), want, 1e-9, f"{e} row {ROWS[c]} summed against physical space")


# ---- closure over two steps ---------------------------------------------------------------------------
DT = 1e-3


def _smooth_state():
    from channel_gpu_amd.reference import budgets as bud

    plan, ops = ora.OraclePlan(16, 65, 9), ora.build_ops(65)
    phi, om = bud.smooth_state(plan, ops, seed=9, amp=0.3)
    return phi, om, 0.75 * 1.8 * (1 - ops.y ** 2)


def closure_residuals(spectra0, spectra1, spectra2, rows, ops, nu, U):
    """Centred differences of the uu, vv, ww, uv spectra over two steps of DT against the right-hand
    sides assembled from the budget rows and the spectra of the middle state, per stress and output:
    max |rate - RHS| over planes [2:-2] and all k, relative to the largest term there."""
    out = {}
    for e in ("ekx", "ekz"):
        rate = (spectra2[e][:4] - spectra0[e][:4]) / (2 * DT)
        T = sbr.budget_terms(ops, nu, U, rows[e], spectra1[e][:4])
        for i, st in enumerate(sbr.STRESSES):
            big = max(np.abs(t[2:-2]).max() for t in T[st].values())
            out[st, e] = np.abs(rate[i] - sum(T[st].values()))[2:-2].max() / big
    return out


# The NumPy reference through the same procedure (16 x 65 x 9, fp64, DT = 1e-3, the smooth state of the CPU
# closure test, budgets.smooth_state(seed=9, amp=0.3); centred differences and the compact operators on this
# state) leaves the residuals REFERENCE_CLOSURE (reference_closure() below, run on the CPU); the bounds are
# three times those, as BALANCE_BOUNDS of tests/test_pstrain_gpu.py.  The state of the other tests,
# random_state, is independent from point to point in y: there the compact derivatives of the reference
# itself leave residuals of 0.3 to 1.5 and a bound from them would show nothing.
REFERENCE_CLOSURE = {
    ("uu", "ekx"): 2.355e-03, ("vv", "ekx"): 2.426e-04, ("ww", "ekx"): 2.187e-03, ("uv", "ekx"): 3.554e-04,
    ("uu", "ekz"): 2.236e-03, ("vv", "ekz"): 2.239e-04, ("ww", "ekz"): 1.240e-03, ("uv", "ekz"): 3.536e-04,
}


def reference_closure():
    """What REFERENCE_CLOSURE records (CPU, a few seconds)."""
    from channel_gpu_amd.reference import spectra as spc

    o = ora.OracleSolver(NX=16, NY=65, NZ=9, Re=RE, dt_fixed=DT)
    o.set_state(*_smooth_state())
    o.prepare()
    sp = [spc.plane_spectra(o)]
    o.step()
    if o.fields is None:
        o.prepare()
    sb = sbr.spectral_budgets(o)
    U = np.array(o.U)
    sp.append(spc.plane_spectra(o))
    o.step()
    if o.fields is None:
        o.prepare()
    sp.append(spc.plane_spectra(o))
    return closure_residuals(sp[0], sp[1], sp[2], sb, o.ops, o.nu, U)


def test_closure_on_the_device(native):
    cfg = default_config(NX=16, NY=65, NZ=9, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=DT)
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.set_state(*_smooth_state())
    s.prepare()
    sp = [s.plane_spectra()]
    s.step(False)
    sb = s.spectral_budgets()
    U = np.asarray(s.mean_profile())
    sp.append(s.plane_spectra())
    s.step(False)
    sp.append(s.plane_spectra())
    res = closure_residuals(sp[0], sp[1], sp[2], sb, ora.build_ops(65), 1.0 / RE, U)
    bad = []
    for key, r in res.items():
        bound = 3.0 * REFERENCE_CLOSURE[key]
        print(f"closure {key[0]} {key[1]}: residual {r:.3e} (reference {REFERENCE_CLOSURE[key]:.3e}, bound {bound:.3e})")
        if not r < bound:
            bad.append(key)
    assert not bad, bad


# ---- non-disturbance, files, communicator -------------------------------------------------------------
def _stepping_solver(native, **kw):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=DT, **kw)
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(32, 33, 17, False)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s


def test_calls_do_not_disturb_the_run(native):
    a = _stepping_solver(native)
    for _ in range(8):
        a.step(False)
    b = _stepping_solver(native)
    for _ in range(4):
        b.step(False)
    before = (b.plane_spectra(True), b.pressure_strain(), b.pressure_moments())
    r1 = b.spectral_budgets()
    r2 = b.spectral_budgets()
    for e in ("ekx", "ekz"):
        for r in range(20):
            _check_row(r2[e][r], r1[e][r], 1e-12, f"{e} row {ROWS[r]} twice")
    after = (b.plane_spectra(True), b.pressure_strain(), b.pressure_moments())
    for e in ("ekx", "ekz"):
        for r in range(8):
            _check_row(after[0][e][r], before[0][e][r], 1e-12, f"plane_spectra(True) {e} row {r} before and after")
    for q in range(7):
        _check_row(after[1][q], before[1][q], 1e-12, f"pressure_strain() row {q} before and after")
    for q in range(4):
        _check_row(after[2][q], before[2][q], 1e-12, f"pressure_moments() row {q} before and after")
    for _ in range(4):
        b.step(False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    assert La.dt == Lb.dt and La.time == Lb.time


def test_files(native, tmp_path):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", sbudget_every=2)
    assert "sbudget_every = 2;" in cfg.to_string()
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    now = s.spectral_budgets()
    p = s.plan
    for step in (2, 4):
        for name, nk in (("KX", p.Kx + 1), ("KZ", p.nkz)):
            a = np.load(tmp_path / f"SBUD_{name}_{step:08d}.npy")
            assert a.shape == (20, 33, nk) and a.dtype == np.dtype("<f8") and np.isfinite(a).all()
        js = json.loads((tmp_path / f"SBUD_{step:08d}.json").read_text())
        assert js["step"] == step and js["rows"] == list(ROWS) and js["Re"] == 1000.0
        assert js["ax"] == p.ax and js["az"] == p.az and js["time"] > 0
        assert np.array_equal(js["y"], np.asarray(s.grid.y))
        assert len(js["U"]) == 33 and len(js["dU"]) == 33
    assert np.array_equal(js["U"], now["U"]) and np.array_equal(js["dU"], now["dU"])
    assert sorted(f.name for f in tmp_path.glob("SBUD_*")) == sorted(
        [f"SBUD_{n}_{st:08d}.npy" for n in ("KX", "KZ") for st in (2, 4)] + [f"SBUD_{st:08d}.json" for st in (2, 4)])
    # the files hold the binary sums; the atomics are unordered, so equal to rounding only
    for name, e in (("KX", "ekx"), ("KZ", "ekz")):
        a = np.load(tmp_path / f"SBUD_{name}_{4:08d}.npy")
        for r in range(20):
            _check_row(a[r], now[e][r], 1e-12, f"file {name} row {ROWS[r]}")


def test_one_rank_communicator(native, monkeypatch, tmp_path, capfd):
    """With a communicator the call is refused like the pressure, and the driver path prints its note
    once and writes no file."""
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    ref = _reference(32, 33, 17, False)
    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0, dt_fixed=DT, path=str(tmp_path) + "/", sbudget_every=1)
    assert c.solver.comm_kind() != "none"
    c.set_state(ref["phi"], ref["om"], ref["U"])
    with pytest.raises(RuntimeError, match="single-rank"):
        c.spectral_budgets()
    with pytest.raises(RuntimeError, match="single-rank"):
        c.solver.rotational_hat()
    capfd.readouterr()
    c.solver.run(3, False)
    err = capfd.readouterr().err
    assert err.count("sbudget_every") == 1 and "skipped" in err
    assert not list(tmp_path.glob("SBUD_*"))


def test_channelflow_and_sampling(native, tmp_path):
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
    c.initialize()
    p = c.solver.plan
    sb = c.spectral_budgets()
    assert sb["ekx"].shape == (20, 33, p.Kx + 1) and sb["ekz"].shape == (20, 33, p.nkz)
    assert np.allclose(sb["kx"], p.ax * np.arange(p.Kx + 1), rtol=1e-15) and np.allclose(sb["kz"], p.az * np.arange(p.nkz), rtol=1e-15)
    r = c.sample_statistics(8, every=4, spectral_budgets=True).spectral_budgets()
    assert c.statistics.nsb == 2
    assert r["y_plus"].shape == (17,) and r["kx_plus"].shape == (p.Kx + 1,) and r["kz_plus"].shape == (p.nkz,)
    from channel_gpu_amd.models.statistics import SBUDGET_STRESSES, SBUDGET_TERMS

    for key, nk in (("x", p.Kx + 1), ("z", p.nkz)):
        for st in SBUDGET_STRESSES:
            for t in SBUDGET_TERMS:
                for k in ("terms_k", "premult_k"):
                    a = r[k + key][st][t]
                    assert a.shape == (17, nk) and np.isfinite(a).all(), (k, key, st, t)
