"""Cross-spectra of every plane against reference planes on the GPU (Solver.plane_cross_spectra: the
ycross kernel) against the NumPy reference (reference/cross_spectra.py) on the oracle's fields, and
against what the solver already has: plane_spectra() at y = y_r.

States and solver set-up as tests/test_yspectra_gpu.py.  Tolerances relative to the maximum of |row| over
all (ref, y, k): 1e-10 in fp64, 1e-5 in fp32 storage (the oracle is given the complex64-rounded phi and
omega), 1e-9 in the combine mode, 1e-12 between two device results (the atomics are unordered)."""
import functools
import json
import os
import tempfile
import time
import uuid

import numpy as np
import pytest
import torch.multiprocessing as mp

from channel_gpu_amd.reference import cross_spectra as xsp
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

RE = 400.0
# at NY = 33: a wall, both sides of a tile boundary, the centre, and the plane alone in the padded last tile
REFS = (0, 7, 8, 16, 32)
SETS = ("velocity", "shear")


def _round32(a):
    return a.astype(np.complex64).astype(complex)


def _state(NX, NY, NZ, fp32=False):
    plan, ops = ora.OraclePlan(NX, NY, NZ), ora.build_ops(NY)
    phi, om = ora.random_state(plan, ops, seed=9, amp=0.3)
    if fp32:
        phi, om = _round32(phi), _round32(om)
    return phi, om, 0.75 * 1.8 * (1 - ops.y ** 2)


@functools.lru_cache(maxsize=None)
def _oracle(NX, NY, NZ, fp32):
    """Oracle state (complex64-rounded for fp32 storage) and the prepared oracle; once per case, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=RE)
    phi, om, U = _state(NX, NY, NZ, fp32)
    o.set_state(phi, om, U)
    o.prepare()
    for a in (phi, om, U):
        a.setflags(write=False)
    return dict(o=o, phi=phi, om=om, U=U)


@functools.lru_cache(maxsize=None)
def _reference(NX, NY, NZ, fp32, refs, rows):
    c = xsp.plane_cross_spectra(_oracle(NX, NY, NZ, fp32)["o"], list(refs), rows)
    c["ckx"].setflags(write=False)
    c["ckz"].setflags(write=False)
    return c


def _solver(native, NX, NY, NZ, precision, **kw):
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=RE, precision=precision, ic="zero", log_every=0, symmetry_every=0,
                         **{"stats_every": 0, **kw})
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _oracle(NX, NY, NZ, precision == "fp32")
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    return s


def _tol(precision):
    return 1e-10 if precision == "fp64" else 1e-5


def _check_row(got, ref, tol, what, scale=None):
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale)
    print(f"{what}: rel. error {err:.3e} (tol {tol:.1e})")
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"


def _check(cs, ref, tol, what):
    """A plane_cross_spectra() result against another one or the reference's, row by row."""
    assert list(cs["rows"]) == list(ref["rows"]) and list(cs["ref_planes"]) == list(ref["ref_planes"])
    for e in ("ckx", "ckz"):
        assert cs[e].dtype == np.complex128 and cs[e].shape == ref[e].shape, e
        for q, name in enumerate(ref["rows"]):
            assert np.abs(ref[e][q]).max() > 0
            _check_row(cs[e][q], ref[e][q], tol, f"{what} {e} row {name}")


def _case(native, NX, NY, NZ, precision, tol, what, refs=REFS, sets=SETS, **kw):
    s = _solver(native, NX, NY, NZ, precision, **kw)
    for rows in sets:
        _check(s.plane_cross_spectra(list(refs), rows), _reference(NX, NY, NZ, precision == "fp32", tuple(refs), rows), tol,
               f"{what} {rows}")
    return s


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("NX", [32, 48])
def test_plain_layout(native, NX, precision):
    s = _case(native, NX, 33, 17, precision, _tol(precision), "plain")
    assert s.spec_kzb() == 0
    p = s.plan
    for rows in SETS:
        a = s.plane_cross_spectra(list(REFS), rows)
        assert a["ckx"].shape == (4, 5, 33, p.Kx + 1) and a["ckz"].shape == (4, 5, 33, p.nkz)
        assert not a["ckx"][..., 0].imag.any()
        # accumulators are reset per call
        _check(a, _reference(NX, 33, 17, precision == "fp32", REFS, rows), _tol(precision), f"plain {rows} (second call)")


def test_blocked_layout_padded(native, monkeypatch):
    """nkz = 11 pads to 16 lines and 33 planes pad to 40: a kernel that reads the padding or drops the
    last partial tile shows."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s = _case(native, 32, 33, 17, "fp64", 1e-10, "blocked")
    assert s.spec_kzb() == 8


def test_blocked_layout_kz_slices(native, monkeypatch):
    """nkz = 86 pads to 88 lines: two 64-line kz slices, the second partial, in fp32 (two elements per
    lane); the 21 kx rows are three kx slices."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s = _case(native, 32, 33, 129, "fp32", 1e-5, "blocked, two kz slices")
    assert s.spec_kzb() == 8 and s.plan.nkz == 86


def test_blocked_layout_natural(native):
    """R = 7: the blocked layout as the headline grid has it, fp32; plane 384 is alone in its chunk."""
    s = _case(native, 16, 385, 9, "fp32", 1e-5, "blocked, R = 7", refs=(0, 191, 192, 384))
    assert s.spec_kzb() == 8


def test_combine_mode(native, monkeypatch):
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s = _case(native, 32, 33, 17, "fp64", 1e-9, "combine")
    assert s.combine()


def test_against_existing_outputs(native):
    """Independent of the new reference: at y = y_r the real parts are rows 0..3 of plane_spectra() (wz_wz:
    row 6) and the imaginary parts of the auto rows vanish to rounding (not exactly: FMA contraction)."""
    s = _solver(native, 32, 33, 17, "fp64")
    sp = s.plane_spectra()
    refs = list(REFS)
    v, sh = s.plane_cross_spectra(refs), s.plane_cross_spectra(refs, "shear")
    for e, k in (("ekx", "ckx"), ("ekz", "ckz")):
        for q in range(4):
            own = np.stack([v[k][q, i, yr] for i, yr in enumerate(refs)])
            scale = np.abs(v[k][q]).max()
            _check_row(own.real, sp[e][q][refs], 1e-12, f"{k} row {v['rows'][q]} at y = y_r against plane_spectra()", scale)
            if q < 3:
                assert np.abs(own.imag).max() < 1e-12 * scale, (k, q)
        own = np.stack([sh[k][3, i, yr] for i, yr in enumerate(refs)])
        scale = np.abs(sh[k][3]).max()
        _check_row(own.real, sp[e][6][refs], 1e-12, f"{k} row wz_wz at y = y_r against plane_spectra()", scale)
        assert np.abs(own.imag).max() < 1e-12 * scale
    # away from y = y_r the imaginary parts are of the size of the rows
    assert np.abs(v["ckx"][0].imag).max() > 0.1 * np.abs(v["ckx"][0]).max()


@pytest.mark.parametrize("rows", SETS)
def test_order_and_number_of_planes(native, rows):
    """The result does not depend on how the reference planes are batched: a permutation of ref_planes
    permutes it, a single plane equals its slice of the five-plane call."""
    s = _solver(native, 32, 33, 17, "fp64")
    refs = list(REFS)
    a = s.plane_cross_spectra(refs, rows)
    perm = [3, 0, 4, 2, 1]
    b = s.plane_cross_spectra([refs[i] for i in perm], rows)
    assert list(b["ref_planes"]) == [refs[i] for i in perm]
    one = s.plane_cross_spectra([refs[2]], rows)
    assert one["ckx"].shape[1] == 1
    for e in ("ckx", "ckz"):
        for q, name in enumerate(a["rows"]):
            scale = np.abs(a[e][q]).max()
            _check_row(b[e][q], a[e][q][perm], 1e-12, f"{e} row {name} permuted", scale)
            _check_row(one[e][q][0], a[e][q][2], 1e-12, f"{e} row {name} single plane", scale)


def test_one_rank_communicator(native, monkeypatch):
    """kx sub-blocks, the reference plane's offset inside a sub-block and the all-reduce: equal to the
    communicator-free solver's result."""
    s = _solver(native, 32, 33, 17, "fp64")
    ref = _oracle(32, 33, 17, False)
    base = {rows: s.plane_cross_spectra(list(REFS), rows) for rows in SETS}
    monkeypatch.setenv("CHANNEL_FORCE_COMM", "1")
    from channel_gpu_amd.models.channel import ChannelFlow

    c = ChannelFlow(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", stats_every=0, log_every=0,
                    symmetry_every=0)
    assert c.solver.comm_kind() != "none"
    c.set_state(ref["phi"], ref["om"], ref["U"])
    p = c.solver.plan
    for rows in SETS:
        cs = c.plane_cross_spectra(REFS, rows)
        _check(cs, base[rows], 1e-12, f"communicator {rows}")
        assert np.allclose(cs["kx"], p.ax * np.arange(p.Kx + 1), rtol=1e-15) and np.allclose(cs["kz"], p.az * np.arange(p.nkz), rtol=1e-15)
        assert np.array_equal(cs["y"], np.asarray(c.solver.grid.y))


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
    out = dict(kx0=p.kx0, kz0=p.kz0)
    for rows in SETS:
        cs = s.plane_cross_spectra(list(REFS), rows)
        out[rows + "_ckx"], out[rows + "_ckz"] = cs["ckx"], cs["ckz"]
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **out)
    del s


def test_four_ranks(native):
    """World 4 as a 2 x 2 pencil over the host shared-memory communicator: kx and kz both split
    (kz0 > 0 occurs), every rank holds the global result."""
    s = _solver(native, 32, 33, 17, "fp64")
    one = {rows: s.plane_cross_spectra(list(REFS), rows) for rows in SETS}
    world, limit = 4, 120.0
    shm = f"shm:chtestyc_{uuid.uuid4().hex[:12]}"
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
        for rows in SETS:
            got = dict(rows=one[rows]["rows"], ref_planes=one[rows]["ref_planes"], ckx=q[rows + "_ckx"], ckz=q[rows + "_ckz"])
            _check(got, one[rows], 1e-12, f"rank {r} of 4 {rows}")


def test_refusals(native):
    s = _solver(native, 32, 33, 17, "fp64")
    for bad in ([], [7, 7], [3, 7, 3], [-1], [33], list(range(17))):
        with pytest.raises(RuntimeError):
            s.plane_cross_spectra(bad)
    with pytest.raises(RuntimeError):
        s.plane_cross_spectra([7], "pressure")
    # 16 planes are accepted, and the solver still works after the refusals
    a = s.plane_cross_spectra(list(range(16)))
    assert a["ckx"].shape[1] == 16
    _check_row(a["ckx"][0, 7], _reference(32, 33, 17, False, REFS, "velocity")["ckx"][0, 1], 1e-10, "plane 7 of 16")


DT = 1e-3


def _stepping_solver(native):
    cfg = default_config(NX=32, NY=33, NZ=17, Re=RE, precision="fp64", ic="zero", log_every=0, symmetry_every=0,
                         stats_every=0, dt_fixed=DT)
    s = native.Solver(cfg, 0, 1, 0, b"")
    ref = _oracle(32, 33, 17, False)
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
    b.plane_cross_spectra(list(REFS))
    b.plane_cross_spectra(list(REFS), "shear")
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
    for rows in SETS:
        _check(b.plane_cross_spectra(list(REFS), rows), xsp.plane_cross_spectra(o, list(REFS), rows), 1e-9, f"after four steps {rows}")


def test_files_and_sampling(native, tmp_path):
    refs = [0, 7, 25, 32]
    cfg = default_config(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0, path=str(tmp_path) + "/", ycross_every=2,
                         ycross_planes=",".join(map(str, refs)), ycross_rows="shear")
    s = native.Solver(cfg, 0, 1, 0, b"")
    s.init_ic()
    s.run(4, False)
    now = s.plane_cross_spectra(refs, "shear")
    p = s.plan
    y = np.asarray(s.grid.y)
    for step in (2, 4):
        for name, nk in (("KX", p.Kx + 1), ("KZ", p.nkz)):
            a = np.load(tmp_path / f"YCROSS_{name}_{step:08d}.npy")
            assert a.shape == (4, 4, 33, nk) and a.dtype == np.dtype("<c16") and np.isfinite(a).all()
        js = json.loads((tmp_path / f"YCROSS_{step:08d}.json").read_text())
        assert js["step"] == step and js["rows"] == ["u_wz", "v_wz", "w_wx", "wz_wz"] and js["row_set"] == "shear"
        assert js["ref_planes"] == refs and np.array_equal(js["ref_y"], y[refs]) and js["Re"] == 1000.0
        assert js["ax"] == p.ax and js["az"] == p.az and js["time"] > 0
        assert np.array_equal(js["y"], y)
    assert sorted(f.name for f in tmp_path.glob("YCROSS_*")) == sorted(
        [f"YCROSS_{n}_{st:08d}.npy" for n in ("KX", "KZ") for st in (2, 4)] + [f"YCROSS_{st:08d}.json" for st in (2, 4)])
    # the files hold the binary sums; the atomics are unordered, so equal to rounding only
    for name, e in (("KX", "ckx"), ("KZ", "ckz")):
        a = np.load(tmp_path / f"YCROSS_{name}_{4:08d}.npy")
        for q in range(4):
            _check_row(a[q], now[e][q], 1e-12, f"file {name} row {now['rows'][q]}")

    from channel_gpu_amd.models.channel import ChannelFlow

    for rows in SETS:
        c = ChannelFlow(NX=32, NY=33, NZ=17, Re=1000.0, precision="fp32", ic="random", ic_amplitude=0.2, stats_every=0,
                        log_every=0, symmetry_every=0, path=str(tmp_path) + "/")
        c.initialize()
        r = c.sample_statistics(8, every=4, cross_spectra=True, cross_planes=refs, cross_rows=rows).cross_correlations()
        assert c.statistics.ncs == 2
        # 0 | 32 and 7 | 25 are folded
        assert list(r["ref_planes"]) == [0, 7] and r["ref_y_plus"].shape == (2,) and r["y_plus"].shape == (33,)
        assert r["r_x_plus"].shape == (32,) and r["r_z_plus"].shape == (32,)
        for row in xsp.row_names(rows):
            for key, shape in (("R_x", (2, 33, 32)), ("R_z", (2, 33, 32)), ("R_y", (2, 33)),
                               ("coherence_kx", (2, 33, p.Kx + 1)), ("coherence_kz", (2, 33, p.nkz))):
                a = r[key][row]
                assert a.shape == shape and np.isfinite(a).all(), (key, row)
            assert np.abs(r["R_x"][row]).max() <= 1 + 1e-6 and r["coherence_kz"][row].max() <= 1 + 1e-6
            fa, fb = xsp.ROW_FACTORS[row]
            if fa == fb:
                assert abs(r["R_y"][row][1, 7] - 1.0) < 1e-10, row
                # (at the wall the velocities vanish: 0, or 1 where rounding has left a variance)
                wall = r["R_y"][row][0, 0]
                assert abs(wall - 1.0) < 1e-10 or (row != "wz_wz" and wall == 0.0), (row, wall)
    with pytest.raises(ValueError):
        c.sample_statistics(4, every=4, cross_spectra=True)
