"""CFL time-step control against independent references: the maxima of the z stage against NumPy
(plane offset y0, non-uniform 1 / dy, distinct kx_max and kz_max, accumulation over calls), the
dt_update kernel against the formulas of COMPAT.md A14, and the solver with an adaptive dt (no
dt_fixed) step by step against the fp64 oracle: logged maxima, dt, time, state and the mean-flow
diagnostics, on the fast path, the y-chunk pipeline, the 1-rank RCCL communicator with kx
sub-blocks, in fp32, and with the reference-compatibility modes cfl_mode / forcing = "parity"."""
import math

import numpy as np
import pytest
import torch

import refchecks as rc
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


# ---- 1. CFL maxima of the z stage ------------------------------------------------------------------
Y0, NY_CHUNK, CX, CZ = 5, 3, 10.0, 21.0


def zstage_fields(seed, NX, Nzp):
    """Random spectral input [6, ny, NX, nkz] of the z stage (as test_kernels_gpu.py::test_zphys) and
    its physical u, v, w from NumPy's fp64 irfft."""
    rng = np.random.default_rng(seed)
    nkz = Nzp // 3 + 1
    f = rng.standard_normal((6, NY_CHUNK, NX, nkz)) + 1j * rng.standard_normal((6, NY_CHUNK, NX, nkz))
    f[..., 0] = f[..., 0].real
    phys = np.fft.irfft(np.concatenate([f[:3], np.zeros(f[:3].shape[:-1] + (Nzp // 2 + 1 - nkz,))], -1), n=Nzp,
                        axis=-1, norm="forward")
    return f, phys


def check_zstage_maxima(native, NX, Nzp, dtype):
    """Shared with the CHANNEL_ZREG=1 child of test_kernels_gpu.py (the register z kernel)."""
    inv_dy = ora.OracleSolver(8, 33, 5).inv_dy  # NY = 33: wall-clustered, 96.6 at the wall, 33.9 at row 5
    f64 = dtype == torch.complex128
    tmax, tsum = (rc.TOL_MAX_F64, rc.TOL_SUM_F64) if f64 else (rc.TOL_CFL_F32, rc.TOL_CFL_F32)
    refs = []
    maxima = torch.zeros(4, dtype=torch.float32, device="cuda")
    for call, seed in enumerate((Nzp, Nzp + 1)):
        f, (u, v, w) = zstage_fields(seed, NX, Nzp)
        rc.assert_cfl_sensitive(u, v, w, inv_dy, Y0, CX, CZ)
        refs.append(rc.cfl_maxima(u, v, w, inv_dy[Y0:Y0 + NY_CHUNK], CX, CZ))
        ft = torch.tensor(f, dtype=dtype, device="cuda")
        # fresh maxima (the default) and the shared tensor, which accumulates over the calls
        _, m1 = native.zphys(ft, Nzp, torch.tensor(inv_dy), CX, CZ, y0=Y0)
        _, m2 = native.zphys(ft, Nzp, torch.tensor(inv_dy), CX, CZ, y0=Y0, maxima=maxima)
        assert m2.data_ptr() == maxima.data_ptr()
        for got, want, what in ((m1.cpu().numpy(), refs[-1], "fresh"), (maxima.cpu().numpy(), np.max(refs, axis=0), "shared")):
            err = np.abs(got - want) / want
            print(f"zphys maxima NX={NX} Nzp={Nzp} {dtype} call {call} {what}: rel err {err}")
            assert (err[:3] < tmax).all() and err[3] < tsum, (what, call, got, want, err)
    # the second call's fields must not be dominated by the first's in every entry, nor dominate them
    assert not (refs[1] >= refs[0]).all() or not (refs[0] >= refs[1]).all()


@pytest.mark.parametrize("NX,Nzp,dtype", [(16, 32, torch.complex128), (8, 128, torch.complex64),
                                          (16, 1024, torch.complex64), (16, 1024, torch.complex128),
                                          (8, 2048, torch.complex64), (4, 1536, torch.complex128)])
def test_zphys_cfl_maxima(native, NX, Nzp, dtype):
    """All four maxima of the z stage on planes y0 = 5 .. 7 of the NY = 33 grid, cx = 10, cz = 21,
    against max(|u| cx + |v| inv_dy[y0 + y] + |w| cz) and the plain maxima of the NumPy fp64 fields;
    a second call on other fields with the same maxima tensor gives the element-wise maximum of both
    (the solver's chunks accumulate like that).  (8, 2048): rows over two waves; (4, 1536): 3 * 2^k."""
    check_zstage_maxima(native, NX, Nzp, dtype)


# ---- 2. dt_update against the formulas ---------------------------------------------------------------
GEOM = dict(NX=32, NZ=17, LX=2 * math.pi, LZ=math.pi, Re=400.0, NY=33)
# another box (ax = 0.75, az = 1.6): on the one above NX / (2 pi LX) = NX / (4 pi^2) and LX = 2 LZ
GEOM_BOX = dict(GEOM, LX=8 * math.pi / 3, LZ=5 * math.pi / 4)


def f32(*x):
    return [float(np.float32(v)) for v in x]


DT_CASES = [
    ("corrected", f32(1.3, 0.2, 0.4, 217.3), dict(), False),
    ("zero sum -> dt_max", f32(0.0, 0.0, 0.0, 0.0), dict(), False),
    ("dt_max clamp", f32(1.3, 0.2, 0.4, 3.7), dict(), False),
    ("dt_fixed", f32(1.3, 0.2, 0.4, 217.3), dict(dt_fixed=1.25e-3), False),
    ("parity dt_c", f32(13.0, 2.0, 4.0, 2173.0), dict(parity=1), False),
    ("parity dt_v", f32(1.3e-3, 2e-4, 4e-4, 0.2173), dict(parity=1, dt_max=10.0), False),
    ("parity dt_max", f32(1.3e-3, 2e-4, 4e-4, 0.2173), dict(parity=1, Re=4000.0), False),
    ("inf sum", f32(1.3, 0.2, 0.4, math.inf), dict(), True),
    ("nan umax", f32(math.nan, 0.2, 0.4, 217.3), dict(), True),
    ("collapsed dt", f32(1.3, 0.2, 0.4, 1e12), dict(), True),
]


@pytest.mark.parametrize("name,maxima,kw,bad", DT_CASES)
def test_dt_update_kernel(native, name, maxima, kw, bad):
    """dt_update_kernel against rc.dt_reference (plain Python from COMPAT.md A14): dt_c, dt_v, their
    minimum under dt_max, the dt_fixed override, time advanced by dt, the maxima reset to exactly 0
    and health bit 1 for non-finite maxima or a dt below 1e-12.  fp64 scalar arithmetic: 1e-14."""
    check_dt_update(native, GEOM, name, maxima, kw, bad)


@pytest.mark.parametrize("name,maxima,kw,bad", DT_CASES)
def test_dt_update_kernel_box(native, name, maxima, kw, bad):
    """The same cases on LX = 8 pi / 3, LZ = 5 pi / 4.  Every case has umax != wmax, so the parity
    formulas with LX and LZ swapped give another dt_c (and dt_v): by >= 1e-2, against the 1e-14 held."""
    a = dict(cfl=0.5, dt_max=0.05, dt_fixed=0.0, parity=0, **GEOM_BOX)
    a.update(kw)
    if a["parity"]:
        assert maxima[0] != maxima[2]
        sw = dict(a, LX=a["LZ"], LZ=a["LX"])
        for got, want in zip(rc.dt_reference(maxima, **sw)[:2], rc.dt_reference(maxima, **a)[:2]):
            assert abs(got - want) >= 1e-2 * want, (name, got, want)
    check_dt_update(native, GEOM_BOX, name, maxima, kw, bad)


def check_dt_update(native, geom, name, maxima, kw, bad):
    a = dict(cfl=0.5, dt_max=0.05, dt_fixed=0.0, parity=0, **geom)
    a.update(kw)
    t0 = 0.734375
    log, health, after = native.dt_update(torch.tensor(maxima, dtype=torch.float32), time0=t0, **a)
    log = log.numpy()
    dt_c, dt_v, dt = rc.dt_reference(maxima, **a)
    if name == "parity dt_c":
        assert dt == dt_c < min(dt_v, a["dt_max"])
    if name == "parity dt_v":
        assert dt == dt_v < min(dt_c, a["dt_max"])
    if name in ("parity dt_max", "dt_max clamp"):
        assert dt == a["dt_max"] < min(dt_c, dt_v) or (dt == a["dt_max"] == dt_v < dt_c)
    print(f"dt_update {name}: log {log}, reference dt_c {dt_c} dt_v {dt_v} dt {dt}")
    assert np.array_equal(log[:4], np.asarray(maxima, dtype=np.float64), equal_nan=True)
    for got, want, what in ((log[4], dt_c, "dt_c"), (log[5], dt_v, "dt_v"), (log[6], dt, "dt"), (log[7], t0 + dt, "time")):
        assert abs(got - want) <= 1e-14 * abs(want), (what, got, want)
    assert np.array_equal(after.numpy(), np.zeros(4, np.float32)) and not np.signbit(after.numpy()).any()
    assert (health & 2 != 0) == bad and health & ~2 == 0, health


# ---- 3. the solver with an adaptive dt against the oracle ------------------------------------------------
def standard_state(o, seed=3, fp32=False):
    phi, om = ora.random_state(o.plan, o.ops, seed=seed, amp=0.3)
    if fp32:
        phi = phi.astype(np.complex64).astype(np.complex128)
        om = om.astype(np.complex64).astype(np.complex128)
    return phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2)


def oracle_prestep_checks(o, chunk=8):
    """Preconditions on the oracle's current (pre-step) state: the CFL sum tells the mutations apart."""
    p = o.plan
    u, v, w = ora.spec_to_phys_full(o.fields[:3], p)
    rc.assert_cfl_sensitive(u, v, w, o.inv_dy, 0, p.ax * p.Kx, p.az * p.Kz, chunk=chunk)


def check_step_log(L, o, dts, precision, diagnostics=True):
    """One step's log against the oracle that has just taken the same step with dt_fixed = L.dt:
    o.maxima are those of the pre-step state, which chose L.dt."""
    tmax, tsum = (rc.TOL_MAX_F64, rc.TOL_SUM_F64) if precision == "fp64" else (rc.TOL_CFL_F32, rc.TOL_CFL_F32)
    got = np.array([L.umax, L.vmax, L.wmax, L.cflsum])
    err = np.abs(got - o.maxima) / o.maxima
    dt_ref = min(o.cfl / o.maxima[3], o.dt_max)
    assert dt_ref < o.dt_max  # (precondition: the CFL limit, not the clamp, sets dt)
    edt = abs(L.dt - dt_ref) / dt_ref
    print(f"step {len(dts)}: dt {L.dt:.10e} (oracle {dt_ref:.10e}, rel {edt:.2e}), maxima rel err {err}")
    assert (err[:3] < tmax).all() and err[3] < tsum, (got, o.maxima, err)
    assert edt < tsum and abs(L.dt_c - dt_ref) < tsum * dt_ref, (L.dt, L.dt_c, dt_ref)
    assert abs(L.time - sum(dts)) <= 1e-14 * sum(dts), (L.time, sum(dts))
    assert L.health == 0
    if diagnostics:
        lo, hi = o.dUdy_walls()
        for g, w_, what in ((L.dUdy_lo, lo, "dUdy_lo"), (L.dUdy_hi, hi, "dUdy_hi"), (L.utau, o.utau(), "utau")):
            assert abs(g - w_) <= 1e-10 * abs(w_), (what, g, w_)
        # the flux constraint: the last substep's flux before the correction plus the pressure
        # gradient's response restores Q
        assert abs(L.flux + L.dpdx * (o.ops.trap @ o.mean_U1) - o.Q) < 1e-11, (L.flux, L.dpdx)


def run_adaptive(s, o, state, precision, nsteps=3):
    phi, om, U = state
    o.set_state(phi, om, U)
    s.set_state(phi, om, U)
    s.prepare()
    o.prepare()
    tol, tolU = (1e-9, 1e-11) if precision == "fp64" else (1e-4, 1e-5)
    dts = []
    for it in range(nsteps):
        oracle_prestep_checks(o)
        s.step(False)
        L = s.log()
        dts.append(L.dt)
        o.dt_fixed = L.dt
        o.step()
        check_step_log(L, o, dts, precision, diagnostics=precision == "fp64")
        gphi, gom, gU = s.get_state()
        e = rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U)
        assert e[0] < tol and e[1] < tol and e[2] < tolU, (it, e)
        if precision == "fp64":
            assert abs(o.ops.trap @ gU - o.Q) < 1e-11
    # (precondition) the step really adapts: consecutive dts differ by >= 1e-4
    assert all(abs(b - a) >= 1e-4 * a for a, b in zip(dts, dts[1:])), dts
    return dts


ADAPTIVE = dict(Re=400.0, cfl=0.5, dt_max=0.05, stats_every=0, log_every=0, symmetry_every=0, ic="zero")


@pytest.mark.parametrize("NX,NY,NZ,precision,env,rccl", [
    (32, 33, 17, "fp64", {}, False),
    (32, 65, 33, "fp64", {}, False),
    (32, 33, 17, "fp64", {"CHANNEL_YCHUNK": "7", "CHANNEL_YSTREAMS": "2"}, False),
    (32, 33, 17, "fp64", {"CHANNEL_KBLOCKS": "2", "CHANNEL_YCHUNK": "4"}, True),
    (32, 33, 17, "fp32", {}, False),
], ids=["fast-33", "fast-65", "ychunk7x2", "rccl-kb2-ychunk4", "fp32"])
def test_adaptive_dt_matches_oracle(native, monkeypatch, NX, NY, NZ, precision, env, rccl):
    """Three steps without dt_fixed (graphs on: steps 2 and 3 replay the captured graph with a new
    device-side dt).  Every step: logged maxima and CFL sum against the oracle's maxima of the same
    pre-step state (2e-7 / 1e-6 in fp64, 1e-4 in fp32), dt = cfl / sum, time = sum of dts, the state
    at the suite's tolerances, wall shear, u_tau and the flux constraint.  The y-chunk pipeline sets
    the chunk's plane offset for 1 / dy (two streams: the split chunks' too), the RCCL case runs the
    P > 1 pipeline with the max-allreduce."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, precision=precision, **ADAPTIVE)
    s = native.Solver(cfg, 0, 1, 0, native.new_unique_id() if rccl else b"")
    if rccl:
        assert s.comm_kind() == "rccl" and s.kblocks() == 2
    o = ora.OracleSolver(NX, NY, NZ, Re=400.0, cfl=0.5, dt_max=0.05)
    run_adaptive(s, o, standard_state(o, fp32=precision == "fp32"), precision)
    assert s.graph_active()


def test_cfl_mode_parity(native):
    """cfl_mode = "parity" (COMPAT.md A14): dt_c from the reference's uniform-dy formula on the
    oracle's plain maxima, its viscous limit dt_v, dt their minimum."""
    NX, NY, NZ = 32, 33, 17
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, precision="fp64", cfl_mode="parity", **ADAPTIVE)
    s = native.Solver(cfg, 0, 1, 0, b"")
    o = ora.OracleSolver(NX, NY, NZ, Re=400.0, cfl=0.5, dt_max=0.05)
    phi, om, U = standard_state(o)
    o.set_state(phi, om, U)
    s.set_state(phi, om, U)
    s.prepare()
    seen = set()
    for it in range(2):
        s.step(False)
        L = s.log()
        o.dt_fixed = L.dt
        o.step()
        dt_c, dt_v, dt = rc.dt_reference(o.maxima, 0.5, 0.05, 0.0, 1, NX, NZ, cfg.LX, cfg.LZ, 400.0, NY)
        print(f"parity step {it}: dt {L.dt} dt_c {L.dt_c} dt_v {L.dt_v}; reference {dt} {dt_c} {dt_v}")
        for g, w_, what in ((L.dt, dt, "dt"), (L.dt_c, dt_c, "dt_c"), (L.dt_v, dt_v, "dt_v")):
            assert abs(g - w_) < 1e-6 * w_, (what, g, w_)
        # (precondition) the parity step is not the corrected one
        assert abs(dt - min(o.cfl / o.maxima[3], o.dt_max)) > 1e-3 * dt
        assert rel(s.get_state()[0], o.phi) < 1e-9
        seen.add(dt == dt_c)
    assert seen  # (which of dt_c / dt_v limits is the state's business; both formulas are checked)


@pytest.mark.parametrize("NX,NY,NZ", [(32, 33, 17), (16, 385, 9)])
def test_forcing_parity_matches_oracle(native, NX, NY, NZ):
    """forcing = "parity" (COMPAT.md "mean forcing", meanUevol.c:201-221): half the flux defect added
    to the interior rows of the solved mean profile, against the oracle's independent form of it;
    state and U for two steps at the suite's fp64 tolerances."""
    dt = 0.01 if NY == 33 else 1e-4
    seed, amp = (3, 0.3) if NY == 33 else (5, 0.05)
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision="fp64", dt_fixed=dt, forcing="parity", stats_every=0,
                         log_every=0, symmetry_every=0, ic="zero")
    s = native.Solver(cfg, 0, 1, 0, b"")
    o = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=dt, forcing="parity")
    phi, om = ora.random_state(o.plan, o.ops, seed=seed, amp=amp)
    # a profile whose flux is not Q, so that the forcing has something to add
    U = 0.7 * 1.8 * (1 - o.ops.y ** 2) * (1 + 0.1 * o.ops.y)
    o.set_state(phi, om, U)
    s.set_state(phi, om, U)
    s.prepare()
    for it in range(2):
        o.step()
        s.step(False)
        gphi, gom, gU = s.get_state()
        e = rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U)
        print(f"forcing parity NY={NY} step {it}: rel err phi {e[0]:.2e} omega {e[1]:.2e} U {e[2]:.2e}")
        assert e[0] < 1e-9 and e[1] < 1e-9 and e[2] < 1e-11, (it, e)
        L = s.log()
        assert abs(L.dpdx - o.mean_C) <= 1e-9 * abs(o.mean_C) and abs(L.flux - o.mean_flux) < 1e-11
    # (precondition) the implicit forcing would have given another profile: 1000 x the tolerance
    oi = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=dt)
    oi.set_state(phi, om, U)
    oi.step()
    oi.step()
    assert rel(oi.U, o.U) > 1e-8
