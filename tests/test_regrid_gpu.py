"""Restart onto another grid on the GPU: the regrid kernel in every device layout, the file and the array
entry points, the ranks, and the continuation of a run after it (README "Restarting on another grid").
Sources are restart files written from NumPy arrays (regridchecks.write_files); the expected state is
reference/regrid.py's."""
import os
import subprocess
import tempfile
import uuid

import numpy as np
import pytest
import torch.multiprocessing as mp

import regridchecks as rc
from channel_gpu_amd.models import orr_sommerfeld as osm
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import regrid as rg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "channel_mi355x")


@pytest.fixture(autouse=True)
def _needs_hdf5(native):
    if not native.hdf5_available():
        pytest.skip("hdf5 missing")


def solver(native, grid, precision="fp64", uid=b"", **kw):
    return native.Solver(rc.config(grid, precision, **kw), 0, 1, 0, uid)


def regridded(native, files, grid, precision="fp64", uid=b"", umean="-", **kw):
    s = solver(native, grid, precision, uid, regrid=True, **kw)
    s.read_restart(files[0], files[1], umean)
    return s


def assert_state_equal(got, ref):
    for a, b, name in zip(got, ref, ("phi", "omega", "U")):
        assert np.array_equal(a, b), name


def assert_state_close(got, ref, tol, what=""):
    for a, b, name in zip(got, ref, ("phi", "omega", "U")):
        m = np.abs(b).max()
        err = rc.maxerr(a, b) / m
        print(f"{what} {name}: {err:.3e} of the maximum (bound {tol:.1e})")
        assert err <= tol, (what, name, err)


# ---- 1. identity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_identity_is_the_plain_restart_bitwise(native, tmp_path, precision):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    plain = solver(native, rc.SMALL, precision)
    plain.read_restart(files[0], files[1], "-")
    s = regridded(native, files, rc.SMALL, precision)
    assert_state_equal(s.get_state(), plain.get_state())
    assert s.time() == 3.7 and s.steps_done() == 12
    out = [str(tmp_path / n) for n in ("oG.h5", "oDDV.h5")]
    s.write_restart(out[0], out[1], "-")
    attrs = native.h5_read_attrs(out[0])
    assert attrs["dt"] == 0.004 and attrs["stretch"] == 2.0 and attrs["time"] == 3.7
    if precision == "fp64":
        assert_state_equal(s.get_state(), rc.source_state())


# ---- 2. x and z only ---------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(rc.SMALL, rc.XZ), (rc.XZ, rc.SMALL)])
def test_xz_only_is_exact(native, tmp_path, monkeypatch, src, dst):
    """Unit rows only: no tolerance.  One source plane per batch (CHANNEL_REGRID_BUDGET_MB=0), and the
    dealiased band of the files holds 1e30, which must not reach the state."""
    monkeypatch.setenv("CHANNEL_REGRID_BUDGET_MB", "0")
    files = rc.write_files(native, tmp_path, rc.source_state(src), src)
    s = regridded(native, files, dst)
    got, ref = s.get_state(), rc.reference(src, dst)
    assert_state_equal(got, ref)
    if dst[0] > src[0]:
        Ks, nkz = src[0] // 3, rc.dims(src)[2]
        for f in got[:2]:
            assert not f[:, Ks + 1:-Ks].any() and not f[:, :, nkz:].any() and f[:, :Ks + 1, :nkz].any()
    assert s.time() == 3.7 and s.steps_done() == 12


# ---- 3. y and stretch --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("fp64", 1e-12), ("fp32", 2e-7)])
def test_y_and_stretch_match_the_reference(native, tmp_path, precision, tol):
    """fp64: W = 6 products with sum |w| <= 3 and one division; fp32 storage: one rounding per component
    (2^-24 = 6e-8 of the value, a complex modulus within 2e-7 of the maximum with the fp64 part)."""
    from channel_gpu_amd.models.channel import ChannelFlow

    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    ref = rc.reference(rc.SMALL, rc.FINE)
    s = regridded(native, files, rc.FINE, precision)
    assert_state_close(s.get_state(), ref, tol, "file")
    # the Python interface: load(regrid=True) without the config key, the stretch given, and the array path
    flow = ChannelFlow(rc.config(rc.FINE, precision))
    flow.load(files[0], files[1], regrid=True, src_stretch=2.0)
    assert_state_equal(flow.get_state(), s.get_state())
    flow2 = ChannelFlow(rc.config(rc.FINE, precision))
    phi, om, U = rc.source_state()
    flow2.regrid_from(phi, om, U, NX=rc.SMALL[0], NY=rc.SMALL[1], NZ=rc.SMALL[2], stretch=rc.SMALL[3])
    assert_state_close(flow2.get_state(), ref, tol, "arrays")
    if precision == "fp64":
        # (file: sum w (N2 f) / N2, arrays: sum w f: the same to round-off, not bitwise)
        assert_state_close(flow2.get_state(), s.get_state(), 1e-12, "arrays vs file")


# ---- 4. layouts and windows --------------------------------------------------------------------------
COARSE = (16, 33, 9, 2.0)
TALL = (32, 385, 17, 2.0)


def test_blocked_layout_from_a_coarse_grid(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.smooth_state(COARSE), COARSE)
    s = regridded(native, files, TALL)
    assert s.spec_kzb() == 8
    assert_state_close(s.get_state(), rc.smooth_reference(COARSE, TALL), 1e-12)


def test_blocked_layout_source_to_plain_target(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.smooth_state(TALL), TALL)
    s = regridded(native, files, COARSE)
    assert s.spec_kzb() == 0
    assert_state_close(s.get_state(), rc.smooth_reference(TALL, COARSE), 1e-12)


def test_blocked_layout_forced_at_ny_49(native, tmp_path, monkeypatch):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    plain = regridded(native, files, rc.FINE).get_state()
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s = regridded(native, files, rc.FINE)
    assert s.spec_kzb() == 8
    assert_state_equal(s.get_state(), plain)


def test_widest_windows_ny_1201_to_33(native, tmp_path):
    src = (16, 1201, 9, 2.0)
    assert native.regrid_table(1201, 2.0, 33, 2.0).max_window() > 200
    files = rc.write_files(native, tmp_path, rc.smooth_state(src), src)
    s = regridded(native, files, COARSE)
    assert_state_close(s.get_state(), rc.smooth_reference(src, COARSE), 1e-12)


def test_one_rank_communicator_sub_blocks_are_bitwise(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    plain = regridded(native, files, rc.FINE).get_state()
    s = regridded(native, files, rc.FINE, uid=native.new_unique_id())
    assert s.kblocks() > 1 and s.comm_kind() == "rccl"
    assert_state_equal(s.get_state(), plain)


def test_lds_poison_is_honoured_bitwise(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    plain = regridded(native, files, rc.FINE).get_state()
    native.set_lds_poison(True)
    try:
        got = regridded(native, files, rc.FINE).get_state()
    finally:
        native.set_lds_poison(False)
    assert_state_equal(got, plain)


# ---- 5. ranks ------------------------------------------------------------------------------------------
def _rank_worker(rank, world, shm, d, src, dst, pr):
    import torch  # noqa: F401

    from channel_gpu_amd import require_native

    C = require_native()
    cfg = rc.config(dst, "fp64", regrid=True, decomposition="pencil" if pr > 1 else "slab", pr=pr)
    s = C.Solver(cfg, rank, world, 0, shm.encode())
    p = s.plan
    assert p.Pr == pr and p.Pr * p.Pc == world
    s.read_restart(os.path.join(d, "src_G.h5"), os.path.join(d, "src_DDV.h5"), "-")
    phi, om, U = s.get_state()
    np.savez(os.path.join(d, f"r{rank}.npz"), phi=phi, om=om, U=U, kx0=p.kx0, kz0=p.kz0, kzb=s.spec_kzb(), time=s.time(),
             ny_loc=p.ny_loc)
    del s


def _assemble(parts, field):
    nkx = sum(q[field].shape[1] for q in parts if int(q["kz0"]) == 0)
    nkz = sum(q[field].shape[2] for q in parts if int(q["kx0"]) == 0)
    out = np.zeros((parts[0][field].shape[0], nkx, nkz), complex)
    for q in parts:
        a, b = int(q["kx0"]), int(q["kz0"])
        out[:, a:a + q[field].shape[1], b:b + q[field].shape[2]] = q[field]
    return out


@pytest.mark.parametrize("world,pr,kzb,src,dst", [(2, 1, "0", rc.SMALL, rc.FINE), (3, 1, "1", rc.FINE, rc.SMALL),
                                                  (4, 2, "0", rc.SMALL, rc.FINE)])
def test_ranks_assemble_to_the_one_rank_regrid(native, monkeypatch, world, pr, kzb, src, dst):
    """Every rank reads the source planes of its own kx (pencil: its kz range of them) and nothing is
    exchanged: 2 slab ranks, 3 slab ranks on the blocked layout (33 planes: 8 / 16 / 9 rows) and a 2 x 2
    pencil give the one-rank state bitwise."""
    with tempfile.TemporaryDirectory() as d:
        files = rc.write_files(native, d, rc.source_state(src), src)
        one = regridded(native, files, dst).get_state()
        monkeypatch.setenv("CHANNEL_SPEC_KZB", kzb)
        shm = f"shm:chregrid_{uuid.uuid4().hex[:12]}"
        mp.start_processes(_rank_worker, args=(world, shm, d, src, dst, pr), nprocs=world, join=True, start_method="spawn")
        parts = [dict(np.load(os.path.join(d, f"r{r}.npz"))) for r in range(world)]
    assert all(int(q["kzb"]) == (8 if kzb == "1" else 0) and float(q["time"]) == 3.7 for q in parts)
    if kzb == "1":
        assert [int(q["ny_loc"]) for q in parts] == [8, 16, 9]
    assert np.array_equal(_assemble(parts, "phi"), one[0]) and np.array_equal(_assemble(parts, "om"), one[1])
    assert np.array_equal(parts[0]["U"], one[2])


# ---- 6. continuation against the oracle ------------------------------------------------------------
def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def test_two_steps_after_regrid_match_the_oracle(native, tmp_path):
    """The bounds of test_solver_gpu.py::test_gpu_matches_oracle_fp64 (and its fixed step for NX = 48)."""
    dst = (48, 49, 25, 2.0)
    dt = 0.01 * 32.0 / 48.0
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    s = regridded(native, files, dst, dt_fixed=dt)
    o = ora.OracleSolver(*dst[:3], Re=400.0, dt_fixed=dt)
    o.set_state(*rc.reference(rc.SMALL, dst))
    s.prepare()
    for it in range(2):
        o.step()
        s.step(False)
        gphi, gom, gU = s.get_state()
        print(f"step {it}: phi {rel(gphi, o.phi):.3e} omega {rel(gom, o.om):.3e} U {rel(gU, o.U):.3e}")
        assert rel(gphi, o.phi) < 1e-9, f"phi step {it}"
        assert rel(gom, o.om) < 1e-9, f"omega step {it}"
        assert rel(gU, o.U) < 1e-11, f"U step {it}"
    assert s.health() == 0


# ---- 7. physics ----------------------------------------------------------------------------------------
def test_ts_wave_keeps_its_growth_rate_across_a_regrid(native, tmp_path):
    """The Tollmien-Schlichting wave of test_physics_gpu.py::test_ts_wave_growth_rate: 500 steps on
    16 x 129 x 9, saved, loaded with regrid on 32 x 193 x 17 and run 1000 steps more.  The growth rate
    over each 250 steps after the regrid stays within 0.01 sigma of the Orr-Sommerfeld eigenvalue.

    Measured on an MI355X: rates / sigma - 1 = +0.0019, -0.0005, -0.0009, -0.0010 over the four intervals
    (the first holds the regrid's transient), against the 0.01 allowed."""
    Re, dt = 7500.0, 0.02
    kw = dict(Re=Re, Q=4.0 / 3.0, dt_fixed=dt)
    src, dst = (16, 129, 9, 2.0), (32, 193, 17, 2.0)
    s = solver(native, src, **kw)
    phi, om, U, c = osm.ts_initial_state(ora.OraclePlan(*src[:3]), ora.build_ops(src[1]), Re, eps=1e-6)
    s.set_state(phi, om, U)
    s.prepare()
    for _ in range(500):
        s.step(False)
    files = [str(tmp_path / n) for n in ("G.h5", "DDV.h5")]
    s.write_restart(files[0], files[1], "-")
    r = regridded(native, files, dst, **kw)
    assert r.steps_done() == 500 and abs(r.time() - 500 * dt) < 1e-9
    r.prepare()
    amps, ts = [np.linalg.norm(r.get_state()[0][:, 1, 0]) / np.sqrt(dst[1])], [0.0]
    for i in range(1000):
        r.step(False)
        if i % 250 == 249:
            # (an r.m.s. over the nodes is not a grid-independent norm; only its growth is used)
            amps.append(np.linalg.norm(r.get_state()[0][:, 1, 0]) / np.sqrt(dst[1]))
            ts.append((i + 1) * dt)
    rates = np.diff(np.log(amps)) / np.diff(ts)
    sigma = c.imag  # alpha = 1
    print(f"sigma = {sigma:.6e}, rates / sigma - 1 = {rates / sigma - 1}")
    assert np.all(np.abs(rates - sigma) < 0.01 * sigma), (rates, sigma)
    assert r.health() == 0


# ---- 8. Poiseuille -------------------------------------------------------------------------------------
def test_poiseuille_parabola_and_flux_survive(native, tmp_path):
    src, dst = (32, 33, 17, 2.0), (32, 49, 17, 1.6)
    NY, nkx, nkz = rc.dims(src)
    z = np.zeros((NY, nkx, nkz), complex)
    Us = 0.75 * 1.8 * (1.0 - rg.tanh_grid(NY, 2.0) ** 2)
    files = rc.write_files(native, tmp_path, (z, z, Us), src)
    s = regridded(native, files, dst, Re=100.0, dt_fixed=0.0)
    y, trap = np.asarray(s.grid.y), np.asarray(s.grid.trap)
    U = s.get_state()[2]
    print(f"U error {np.abs(U - 1.35 * (1 - y * y)).max():.3e}, flux error {abs(trap @ U - 1.8):.3e}")
    assert np.abs(U - 0.75 * 1.8 * (1 - y * y)).max() <= 1e-13
    assert abs(trap @ U - 1.8) <= 1e-12  # (the quadrature is cubic-exact: grid.hpp)
    s.prepare()
    for _ in range(10):
        s.step(False)
    U = np.asarray(s.mean_profile())
    # the tolerance of test_solver_gpu.py::test_poiseuille_steady
    assert np.max(np.abs(U - 1.35 * (1 - y * y))) < 1e-10
    assert abs(trap @ U - 1.8) < 1e-10
    assert s.log().health == 0


# ---- 9. the first time step ----------------------------------------------------------------------------
def test_first_adaptive_dt_is_that_of_a_fresh_solver(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    kw = dict(dt_fixed=0.0, cfl=0.5, dt_max=0.05)
    s = regridded(native, files, rc.FINE, **kw)
    fresh = solver(native, rc.FINE, **kw)
    fresh.set_state(*s.get_state())
    dts = []
    for q in (s, fresh):
        q.prepare()
        q.step(False)
        dts.append(q.log().dt)
    assert dts[0] == dts[1] and 0 < dts[0] < 0.05
    assert abs(s.time() - (3.7 + dts[0])) < 1e-12
    assert_state_equal(s.get_state(), fresh.get_state())


# ---- 10. refusals ----------------------------------------------------------------------------------------
def test_mismatched_grid_without_the_key_is_refused_as_before(native, tmp_path):
    """Today's two messages: a file with fewer kx planes than the solver reads fails in the plane read,
    any other mismatch in read_restart's check of the dims."""
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    with pytest.raises(RuntimeError, match=r"io\.cpp:\d+: plane index out of range$"):
        solver(native, rc.FINE).read_restart(files[0], files[1], "-")
    with pytest.raises(RuntimeError, match=r"restart file .*src_G\.h5 has dims 32x33x34$"):
        solver(native, (32, 49, 17, 2.0)).read_restart(files[0], files[1], "-")
    big = rc.write_files(native, tmp_path, rc.source_state(rc.FINE), rc.FINE, name="big")
    with pytest.raises(RuntimeError, match=r"restart file .*big_G\.h5 has dims 48x49x50$"):
        solver(native, rc.SMALL).read_restart(big[0], big[1], "-")


def test_another_box_is_refused_with_both_values(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL, box=dict(LX=2 * np.pi * 1.01, LZ=np.pi))
    s = solver(native, rc.FINE, regrid=True)
    with pytest.raises(RuntimeError) as e:
        s.read_restart(files[0], files[1], "-")
    assert "LX = 6.34601" in str(e.value) and "LX = 6.28318" in str(e.value)


def test_umean_of_the_wrong_length_is_refused(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    um = str(tmp_path / "U49.bin")
    native.umean_write(um, list(np.ones(49)))
    s = solver(native, rc.FINE, regrid=True)
    with pytest.raises(RuntimeError, match="49 records.*NY = 33"):
        s.read_restart(files[0], files[1], um)
    # the source's own length is taken, in the files' N2 units, and wins over the profile inside G
    um33 = str(tmp_path / "U33.bin")
    N2 = rc.SMALL[0] * (2 * rc.SMALL[2] - 2)
    native.umean_write(um33, list(2.0 * N2 * np.ones(33)))
    s.read_restart(files[0], files[1], um33)
    assert np.abs(s.get_state()[2] - 2.0).max() < 1e-13


def test_no_stretch_in_the_file_notes_it_and_takes_the_configs(native, tmp_path, capfd):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL, stretch_attr=False)
    s = regridded(native, files, rc.FINE)
    err = capfd.readouterr().err
    assert err.count("carries no stretch") == 1 and "1.6" in err
    explicit = regridded(native, files, rc.FINE, regrid_stretch=1.6)
    assert "carries no stretch" not in capfd.readouterr().err
    assert_state_equal(s.get_state(), explicit.get_state())
    # and it is not what the file's true stretch gives
    assert not np.array_equal(s.get_state()[0], regridded(native, files, rc.FINE, regrid_stretch=2.0).get_state()[0])


def test_files_without_attributes_are_on_the_configs_box(native, tmp_path):
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL, attrs={}, umean_in_g=False)
    s = regridded(native, files, rc.FINE, regrid_stretch=2.0)
    ref = rc.reference(rc.SMALL, rc.FINE)
    assert_state_close(s.get_state()[:2], ref[:2], 1e-12)
    y = np.asarray(s.grid.y)
    assert np.array_equal(s.get_state()[2], 0.75 * 1.8 * (1.0 - y * y))  # no U anywhere: today's parabola
    assert s.time() == 0.0 and s.steps_done() == 0


# ---- 11. driver ------------------------------------------------------------------------------------------
CONF = """application:
{{
  NX = 48; NY = 49; NZ = 25;
  input: {{ G = "{g}"; DDV = "{ddv}"; UMEAN = "-"; }};
  output: {{ G = "{d}/G.h5"; DDV = "{d}/DDV.h5"; UMEAN = "{d}/Umean.bin"; }};
  path = "{d}/";
  Re = 400.0; nsteps = 2; stats_every = 0; log_every = 1; precision = "fp64"; dt_fixed = 0.005;
  stretch = 1.6; regrid = true;
}};
"""


def test_driver_starts_from_a_restart_on_another_grid(native, tmp_path):
    if not os.path.exists(BIN):
        pytest.skip("driver not built")
    files = rc.write_files(native, tmp_path, rc.source_state(), rc.SMALL)
    d = str(tmp_path / "run")
    os.makedirs(d)
    conf = os.path.join(d, "run.conf")
    with open(conf, "w") as f:
        f.write(CONF.format(g=files[0], ddv=files[1], d=d))
    r = subprocess.run([BIN, conf, "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, dims = native.h5_read_planes(os.path.join(d, "G.h5"), [0])
    assert dims == [48, 49, 50]
    attrs = native.h5_read_attrs(os.path.join(d, "G.h5"))
    assert attrs["stretch"] == 1.6 and attrs["step"] == 14.0 and abs(attrs["time"] - 3.71) < 1e-12
