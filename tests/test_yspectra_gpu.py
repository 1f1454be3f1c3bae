"""One-dimensional spectra and co-spectra at every plane on the GPU (Solver.plane_spectra: the
yspectra kernel) against the NumPy reference (reference/spectra.py) on the oracle's fields, and
against what the solver already has: spectra() at its planes, gradient_sums(), stats(),
pressure_strain().

Tolerances as tests/test_budgets_gpu.py, relative to the maximum of a row over all (y, k): 1e-10 in
fp64, 1e-5 in fp32 storage (the oracle is given the complex64-rounded phi and omega), 1e-9 in the
combine mode, 1e-12 between two device results (the atomics are unordered)."""
import functools
import json
import os
import tempfile
import time
import uuid

import numpy as np
import pytest
import torch.multiprocessing as mp

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import spectra as spc
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0
ROWS = spc.SPECTRA_ROWS


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
    """Oracle state (complex64-rounded for fp32 storage), the prepared oracle and its spectra;
    computed once per case, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om, U = _state(NX, NY, NZ, fp32)
    o.set_state(phi, om, U)
    o.prepare()
    sp = spc.plane_spectra(o)
    for a in (phi, om, U, sp["ekx"], sp["ekz"]):
        a.setflags(write=False)
    return dict(o=o, phi=phi, om=om, U=U, ekx=sp["ekx"], ekz=sp["ekz"])


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


def _check(sp, ref, tol, what, rows=range(7)):
    """Rows of a plane_spectra() result against ref["ekx"], ref["ekz"]."""
    assert list(sp["rows"]) == list(ROWS)
    for e in ("ekx", "ekz"):
        assert sp[e].dtype == np.float64 and sp[e].shape == ref[e].shape, e
        for r in rows:
            _check_row(sp[e][r], ref[e][r], tol, f"{what} {e} row {ROWS[r]}")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_plain_layout(native, NX, precision):
    s, ref = _solver(native, NX, 33, 17, precision)
    assert s.spec_kzb() == 0
    sp = s.plane_spectra()
    p = s.plan
    assert sp["ekx"].shape == (8, 33, p.Kx + 1) and sp["ekz"].shape == (8, 33, p.nkz)
    _check(sp, ref, _tol(precision), "plain")
    assert not sp["ekx"][7].any() and not sp["ekz"][7].any()
    # accumulators are reset per call
    _check(s.plane_spectra(), ref, _tol(precision), "plain (second call)")


def test_blocked_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 planes pad to 40: a kernel that reads the padding or drops the
    last partial tile shows."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.spec_kzb() == 8
    _check(s.plane_spectra(), ref, 1e-10, "blocked")


def test_blocked_layout_kz_slices(native, monkeypatch):
    """nkz = 86 pads to 88 lines: two 64-line kz slices, the second partial, in fp32 (two elements per
    lane); the 21 kx rows are three kx slices, the middle one with +kx and -kx of the same bins."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s, ref = _solver(native, 32, 33, 129, "fp32")
    assert s.spec_kzb() == 8 and s.plan.nkz == 86
    _check(s.plane_spectra(), ref, 1e-5, "blocked, two kz slices")


def test_blocked_layout_natural(native):
    """R = 7: the blocked layout as the headline grid has it, fp32; plane 384 is alone in its chunk."""
    s, ref = _solver(native, 16, 385, 9, "fp32")
    assert s.spec_kzb() == 8
    _check(s.plane_spectra(), ref, 1e-5, "blocked, R = 7")


def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s, ref = _solver(native, 32, 33, 17, "fp64")
    assert s.combine()
    _check(s.plane_spectra(), ref, 1e-9, "combine")


def test_against_existing_outputs(native):
    """Independent of the new reference: spectra() at its planes, gradient_sums(), stats()."""
    planes = [0, 7, 8, 16, 32]
    s, _ = _solver(native, 32, 33, 17, "fp64", spectra_planes=",".join(map(str, planes)), stats_every=1)
    sp = s.plane_spectra()
    old = s.spectra()
    assert list(old["planes"]) == planes
    for e in ("ekx", "ekz"):
        for r in range(3):
            _check_row(sp[e][r][planes], old[e][r], 1e-12, f"{e} row {ROWS[r]} against spectra()", np.abs(sp[e][r]).max())
    g = s.gradient_sums()
    st = np.asarray(s.stats()).reshape(4, 33)
    for e in ("ekx", "ekz"):
        for r in range(3):
            _check_row(sp[e][4 + r].sum(axis=-1), g[r], 1e-12, f"{e} row {ROWS[4 + r]} summed against gradient_sums()")
        _check_row(sp[e][3].sum(axis=-1), st[3], 1e-12, f"{e} row uv summed against stats()")


def test_one_rank_communicator(native, monkeypatch):
    """kx sub-blocks and the all-reduce: equal to the communicator-free solver's result; the pressure
    row is refused."""
    s, ref = _solver(native, 32, 33, 17, "fp64")
    sp0 = s.plane_spectra()
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0)
    assert c.solver.comm_kind() != "none"
    c.set_state(ref["phi"], ref["om"], ref["U"])
    sp = c.plane_spectra()
    _check(sp, sp0, 1e-12, "communicator")
    p = c.solver.plan
    assert np.allclose(sp["kx"], p.ax * np.arange(p.Kx + 1), rtol=1e-15) and np.allclose(sp["kz"], p.az * np.arange(p.nkz), rtol=1e-15)
    with pytest.raises(RuntimeError, match="single-rank"):
        c.plane_spectra(pressure=True)


def _worker(rank, world, shm, outdir, pr):
    import torch  # noqa: F401

    from channel_gpu_amd import require_native

    C = require_native()
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", stats_every=0, log_every=0,
                         symmetry_every=0, decomposition="pencil", pr=pr)
    s = C.Solver(cfg, rank, world, 0, shm.encode())
    p = s.plan
    assert p.Pr == pr and p.Pr * p.Pc == world
    phi, om, U = _state(32, 33, 17)
    sl = slice(p.kx0, p.kx0 + p.nkx_loc)
    sz = slice(p.kz0, p.kz0 + p.nkz_loc)
    s.set_state(np.ascontiguousarray(phi[:, sl, sz]), np.ascontiguousarray(om[:, sl, sz]), U)
    s.prepare()
    sp = s.plane_spectra()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), ekx=sp["ekx"], ekz=sp["ekz"], kx0=p.kx0, kz0=p.kz0)
    del s


def test_four_ranks(native):
    """World 4 as a 2 x 2 pencil over the host shared-memory communicator: kx and kz both split
    (kz0 > 0 occurs), every rank holds the global result."""
    s, _ = _solver(native, 32, 33, 17, "fp64")
    one = s.plane_spectra()
    world, limit = 4, 120.0
    shm = f"shm:chtestys_{uuid.uuid4().hex[:12]}"
    with tempfile.TemporaryDirectory() as d:
        ctx = mp.start_processes(_worker, args=(world, shm, d, 2), nprocs=world, join=False, start_method="spawn")
        t0 = time.monotonic()
        try:
            while not ctx.join(timeout=1.0):
                assert time.monotonic() - t0 < limit, f"a rank did not finish within {limit:.0f} s"
        finally:
            for q in ctx.processes:
                if q.is_alive():
                    q.kill()
        parts = [dict(np.load(os.path.join(d, f"r{r}.npz"))) for r in range(world)]
    assert any(int(q["kz0"]) > 0 for q in parts) and any(int(q["kx0"]) > 0 for q in parts)
    for r, q in enumerate(parts):
        _check(dict(rows=ROWS, ekx=q["ekx"], ekz=q["ekz"]), one, 1e-12, f"rank {r} of 4")


def test_pressure_row(native):
    s, ref = _solver(native, 32, 33, 17, "fp64")
    sp0 = s.plane_spectra()
    sp = s.plane_spectra(pressure=True)
    want = spc.plane_spectra(ref["o"], s.static_pressure_hat())
    _check(sp, want, 1e-10, "pressure", rows=[7])
    assert np.abs(want["ekx"][7]).max() > 0
    ps = s.pressure_strain()
    for e in ("ekx", "ekz"):
        _check_row(sp[e][7].sum(axis=-1), ps[6], 1e-12, f"{e} row pp summed against pressure_strain() pp_band")
    # the other rows are unchanged by the flag, and the row is zero again without it
    _check(sp, sp0, 1e-12, "with and without the pressure row")
    again = s.plane_spectra()
    assert not again["ekx"][7].any() and not again["ekz"][7].any()


DT = 1e-3


def _stepping_solver(native):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=DT)
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _reference(32, 33, 17, False)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s, ref


def test_calls_do_not_disturb_the_run(native):
    a, ref = _stepping_solver(native)
    for _ in range(4):
        a.step(False)
    b, _ = _stepping_solver(native)
    for _ in range(2):
        b.step(False)
    b.plane_spectra(True)
    for _ in range(2):
        b.step(False)
    assert a.graph_active() and b.graph_active()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    La, Lb = a.log(), b.log()
    assert La.dt == Lb.dt and La.time == Lb.time
    # after graph-replayed steps: against the stepped oracle
    o = ora.OracleSolver(NX=32, NY=33, NZ=17, Re=RE, dt_fixed=DT)
    o.set_state(ref["phi"], ref["om"], ref["U"])
    for _ in range(4):
        o.step()
    _check(b.plane_spectra(True), spc.plane_spectra(o), 1e-9, "after four steps")


def test_files_and_sampling(native, tmp_path):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", yspectra_every=2)
    assert "yspectra_every = 2;" in cfg.to_string()
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    now = s.plane_spectra()
    p = s.plan
    for step in (2, 4):
        for name, nk in (("KX", p.Kx + 1), ("KZ", p.nkz)):
            a = np.load(tmp_path / f"YSPEC_{name}_{step:08d}.npy")
            assert a.shape == (8, 33, nk) and a.dtype == np.dtype("<f8") and np.isfinite(a).all()
        js = json.loads((tmp_path / f"YSPEC_{step:08d}.json").read_text())
        assert js["step"] == step and js["rows"] == list(ROWS) and js["Re"] == 1000.0
        assert js["ax"] == p.ax and js["az"] == p.az and js["time"] > 0
        assert np.array_equal(js["y"], np.asarray(s.grid.y))
    assert sorted(f.name for f in tmp_path.glob("YSPEC_*")) == sorted(
        [f"YSPEC_{n}_{st:08d}.npy" for n in ("KX", "KZ") for st in (2, 4)] + [f"YSPEC_{st:08d}.json" for st in (2, 4)])
    # the files hold the binary sums; the atomics are unordered, so equal to rounding only
    for name, e in (("KX", "ekx"), ("KZ", "ekz")):
        a = np.load(tmp_path / f"YSPEC_{name}_{4:08d}.npy")
        for r in range(7):
            _check_row(a[r], now[e][r], 1e-12, f"file {name} row {ROWS[r]}")
        assert not a[7].any()

    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                    log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
    c.initialize()
    r = c.sample_statistics(8, every=4, spectra=True).spectra()
    assert c.statistics.nsp == 2
    assert r["y_plus"].shape == (17,) and r["kx_plus"].shape == (p.Kx + 1,) and r["kz_plus"].shape == (p.nkz,)
    for row in ROWS:
        for key, nk, n in (("x", p.Kx + 1, 32), ("z", p.nkz, 32)):
            for k in ("E_k", "premult_k"):
                a = r[k + key][row]
                assert a.shape == (17, nk) and np.isfinite(a).all(), (k, key, row)
            if row != "uv":
                a = r["R_" + key][row]
                assert a.shape == (17, n // 2 + 1) and np.isfinite(a).all(), (key, row)
