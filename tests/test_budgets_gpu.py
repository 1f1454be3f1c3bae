"""Velocity-gradient sums (Solver.gradient_sums: the spectral reduction kernel) and the triple products
of the turbulent transport (Solver.transport_moments: the export stage) against the NumPy reference
(reference/budgets.py) on the oracle's fields.

fp32 storage: the oracle is given the complex64-rounded phi and omega, so the rounding of the state is
shared (the blocked-layout export test documents 8.9e-6 in v from that rounding alone at NY = 385).
Tolerances are relative to each row's maximum: 1e-10 in fp64, 1e-5 in fp32; the rows formed from
complex64-rounded oracle fields (the emulation of the fp32 storage of K-SPEC's outputs) are within
5.4e-8 (gradient rows) and 2.9e-8 (triple rows) of the unrounded ones, printed by every fp32 case."""
import copy
import functools

import numpy as np
import pytest

from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0


def _round32(a):
    return a.astype(np.complex64).astype(complex)


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32):
    """Oracle state (complex64-rounded for fp32 storage), its gradient sums [7, NY], physical fields
    [6, NY, NX, Nzp] and triple products [3, NY]; computed once per case, read-only.  Also the fp32
    emulation errors of the gradient and triple rows (relative to each row's maximum)."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    if fp32:
        phi, om = _round32(phi), _round32(om)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    grad = bud.gradient_sums(o)
    ph = ora.spec_to_phys_full(o.fields, o.plan)
    tri = bud.transport_moments(ph, U)
    o32 = copy.copy(o)
    o32.fields = _round32(o.fields)
    eg = np.abs(bud.gradient_sums(o32) - grad).max(axis=1) / np.abs(grad).max(axis=1)
    et = np.abs(bud.transport_moments(ph.astype(np.float32).astype(float), U) - tri).max(axis=1) / np.abs(tri).max(axis=1)
    for a in (phi, om, U, grad, ph, tri, eg, et):
        a.setflags(write=False)
    return dict(phi=phi, om=om, U=U, grad=grad, ph=ph, tri=tri, emu_grad=eg, emu_tri=et)


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


def _check_rows(got, ref, tol, names, what):
    assert got.shape == ref.shape and np.isfinite(got).all()
    for r, n in enumerate(names):
        err = np.abs(got[r] - ref[r]).max() / np.abs(ref[r]).max()
        print(f"{what} row {n}: rel. error {err:.3e} (tol {tol:.1e})")
        assert err < tol, f"{what} row {n}: {err:.3e} >= {tol:.1e}"


def _print_emulation(ref, key):
    print(f"fp32 emulation error of the {key} rows:", " ".join(f"{x:.1e}" for x in ref[key]))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_gradient_rows_plain_layout(native, NX, precision):
    s, ref = _solver(native, NX, 33, 17, precision)
    assert s.spec_kzb() == 0
    if precision == "fp32":
        _print_emulation(ref, "emu_grad")
    g = s.gradient_sums()
    assert g.shape == (7, 33) and g.dtype == np.float64
    _check_rows(g, ref["grad"], _tol(precision), bud.GRADIENT_ROWS, "gradient")
    # accumulators are reset per call
    _check_rows(s.gradient_sums(), ref["grad"], _tol(precision), bud.GRADIENT_ROWS, "gradient (second call)")


def test_gradient_rows_tiled_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 rows pad to 40: a kernel that reads the padding or drops the
    last partial tile shows."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check_rows(s.gradient_sums(), ref["grad"], 1e-10, bud.GRADIENT_ROWS, "gradient")


def test_gradient_rows_tiled_layout_natural(native):
    """R = 7: the blocked layout as the headline grid has it, fp32 (two elements per lane)."""
    s, ref = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    _print_emulation(ref, "emu_grad")
    _check_rows(s.gradient_sums(), ref["grad"], 1e-5, bud.GRADIENT_ROWS, "gradient")


def test_gradient_rows_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check_rows(s.gradient_sums(), ref["grad"], 1e-9, bud.GRADIENT_ROWS, "gradient")


def test_one_rank_communicator(native, monkeypatch):
    """kx sub-blocks and the all-reduce: equal to the communicator-free solver's sums (atomics are
    unordered: 1e-12, not bitwise); the triple products are refused."""
    s, ref = _solver(native, 32, 33, 17, "fp64")
    g0 = s.gradient_sums()
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0)
    assert c.solver.comm_kind() != "none"
    c.set_state(ref["phi"], ref["om"], ref["U"])
    _check_rows(c.gradient_sums(), g0, 1e-12, bud.GRADIENT_ROWS, "gradient (communicator)")
    with pytest.raises(RuntimeError, match="single-rank"):
        c.transport_moments()


def test_vorticity_rows_against_physical_fields(native):
    """Independent of the reference formulas: rows 0..2 are the plane means of the squares of the
    exported vorticity fluctuations."""
    s, _ = _solver(native, 32, 33, 17, "fp64")
    g = s.gradient_sums()
    f = s.physical_fields(list(range(33)), ["wx", "wy", "wz"])
    for r, n in enumerate(["wx", "wy", "wz"]):
        a = f[n]
        if n == "wz":
            a = a - a.mean(axis=(1, 2), keepdims=True)  # (-dU/dy)
        ms = (a * a).mean(axis=(1, 2))
        err = np.abs(g[r] - ms).max() / ms.max()
        print(f"<{n}^2>: rel. error {err:.3e}")
        assert err < 1e-10


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [48, 32])
def test_transport_rows(native, NX, precision):
    """NX = 48 rows per plane against 128-row blocks: the blocks straddle planes.  The moments are
    unchanged by the triple-product pass."""
    s, ref = _solver(native, NX, 33, 17, precision)
    if precision == "fp32":
        _print_emulation(ref, "emu_tri")
    m0 = s.plane_moments()
    t = s.transport_moments()
    m1 = s.plane_moments()
    assert t.shape == (3, 33) and t.dtype == np.float64
    _check_rows(t, ref["tri"], _tol(precision), bud.TRANSPORT_ROWS, "transport")
    assert m0.shape == (11, 33) and m1.shape == (11, 33)
    # (row 0, the mean of u', is zero to rounding: held against max |U| as in the moments' own test)
    scale = np.abs(m0).max(axis=1)
    scale[0] = np.abs(ref["U"]).max()
    assert (np.abs(m1 - m0).max(axis=1) <= 1e-13 * scale).all()
    # <v^3>, the fourth transport term, stays row 6 of the moments
    vvv = (ref["ph"][1] ** 3).mean(axis=(1, 2))
    assert np.abs(m0[6] - vvv).max() < _tol(precision) * np.abs(vvv).max()


DT = 1e-3


def _stepping_solver(native):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=DT)
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(32, 33, 17, False)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s, ref


def test_after_graph_replayed_steps(native):
    s, ref = _stepping_solver(native)
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=RE, dt_fixed=DT)
    o.set_state(ref["phi"], ref["om"], ref["U"])
    for _ in range(4):
        o.step()
        s.step(False)
    assert s.graph_active()
    _check_rows(s.gradient_sums(), bud.gradient_sums(o), 1e-9, bud.GRADIENT_ROWS, "gradient")
    tri = bud.transport_moments(ora.spec_to_phys_full(o.fields, o.plan), o.U)
    _check_rows(s.transport_moments(), tri, 1e-9, bud.TRANSPORT_ROWS, "transport")


def test_calls_do_not_disturb_the_run(native):
    a, _ = _stepping_solver(native)
    for _ in range(4):
        a.step(False)
    b, _ = _stepping_solver(native)
    for _ in range(2):
        b.step(False)
    b.gradient_sums()
    b.transport_moments()
    for _ in range(2):
        b.step(False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    assert La.dt == Lb.dt and La.time == Lb.time


def test_energy_balance(native):
    """The CPU test's balance dK/dt = int (P_k - eps_k) dy on the solver itself (fp64): K from stats(),
    eps from gradient_sums(), central difference over two steps about the middle state."""
    dt = 1e-3
    cfg = default_config(NX=32, NY=33, NZ=17, Re=100.0, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=1, dt_fixed=dt)
    s = native.Solver(cfg, 0, 1, 0, b"")
    plan = ora.OraclePlan(32, 33, 17)
    ops = ora.build_ops(33)
    phi, om = bud.smooth_state(plan, ops, seed=3, amp=0.05, kscale=4)
    s.set_state(phi, om, 0.75 * 1.8 * (1 - ops.y ** 2))
    s.prepare()
    K = lambda: 0.5 * ops.trap @ np.asarray(s.stats()).reshape(4, 33)[:3].sum(axis=0)  # noqa: E731
    K0 = K()
    s.step(True)
    st = np.asarray(s.stats()).reshape(4, 33)
    g = s.gradient_sums()
    U = np.asarray(s.mean_profile())
    prod = ops.trap @ (-st[3] * (ops.D1 @ U))
    eps = ops.trap @ ((g[3] + g[4] + g[5]) / 100.0)
    s.step(True)
    K2 = K()
    dK = (K2 - K0) / (2 * dt)
    err = abs(dK - (prod - eps)) / eps
    print(f"dK/dt {dK:.6e}  P {prod:.6e}  eps {eps:.6e}  P/eps {prod / eps:.3f}  |difference| / eps {err:.2e}")
    assert prod > 0.2 * eps
    assert err < 2e-3


def test_files_and_sampled_profiles(native, tmp_path):
    Re = 1000.0
    cfg = default_config(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", budget_every=2)
    assert "budget_every = 2;" in cfg.to_string()
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    g, t = s.gradient_sums(), s.transport_moments()
    want = {"WXRMS": np.sqrt(g[0]), "WYRMS": np.sqrt(g[1]), "WZRMS": np.sqrt(g[2]),
            "EPS_UU": 2 / Re * g[3], "EPS_VV": 2 / Re * g[4], "EPS_WW": 2 / Re * g[5], "EPS_UV": 2 / Re * g[6],
            "TRIPLE_UUV": t[0], "TRIPLE_WWV": t[1], "TRIPLE_UVV": t[2]}
    for name, now in want.items():
        rows = np.loadtxt(tmp_path / f"{name}.dat")
        assert rows.shape == (2, 33) and np.isfinite(rows).all(), name
        # (nine significant digits in the files; the sums are atomics, equal to rounding only)
        assert np.abs(rows[1] - now).max() <= 2e-8 * np.abs(now).max(), name

    from channel_gpu_amd.models.channel import ChannelFlow
    from channel_gpu_amd.models.statistics import BUDGET_STRESSES, BUDGET_TERMS

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=Re, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
    c.initialize()
    p = c.sample_statistics(8, every=4, budgets=True).profiles()
    assert c.statistics.nb == 2
    for k in ["wx_rms", "wy_rms", "wz_rms"] + [f"{t_}_{s_}" for s_ in BUDGET_STRESSES for t_ in BUDGET_TERMS]:
        assert k in p and p[k].shape == (17,) and np.isfinite(p[k]).all(), k
    assert np.array_equal(p["prod_vv"], np.zeros(17))
