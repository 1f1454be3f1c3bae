"""Plane statistics <uu>, <vv>, <ww>, <uv>(y) of the GPU solver against oracle.plane_stats().

Two entry points: prepare() with stats_every = 1 (K-SPEC mode 0: the statistics of exactly the state
given, no time-stepping error) and step(True) (mode 1 at the last substep: the statistics of the new
state, compared after the oracle's step).  Each row is compared as a vector over y (refchecks.py:
stats_errors, stats_tol).  The cases cover the rows-per-lane geometries from NY = 33 to 1201, lines
over two waves, the blocked layout with padded kz lines, the combine mode, kx sub-block launches
accumulating into one buffer; test_multirank_gpu.py adds the sum-allreduce and pencil ranks with
kz0 > 0, test_switches_gpu.py the opt-in K-SPEC variants."""
import functools

import numpy as np
import pytest

import refchecks as rc
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

DT = 1e-4


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def reference(NX, NY, NZ, precision, seed=5, amp=0.05):
    """The oracle's statistics of the standard random state (fp32: rounded through complex64) and
    after one step of dt = 1e-4, computed once per grid and shared (read-only) by the cases."""
    o = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=DT)
    phi, om = ora.random_state(o.plan, o.ops, seed=seed, amp=amp)
    if precision == "fp32":
        phi = phi.astype(np.complex64).astype(np.complex128)
        om = om.astype(np.complex64).astype(np.complex128)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    rc.assert_stats_sensitive(o)
    st0 = o.plane_stats()
    o.step()
    rc.assert_stats_sensitive(o)
    out = dict(phi=phi, om=om, U=U, st0=st0, st1=o.plane_stats(), phi1=o.phi, om1=o.om, U1=o.U)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_stats(native, NX, NY, NZ, precision, uid=b"", seed=5, amp=0.05):
    ref = reference(NX, NY, NZ, precision, seed, amp)
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision=precision, dt_fixed=DT, stats_every=1, log_every=0,
                         symmetry_every=0, ic="zero")
    s = native.Solver(cfg, 0, 1, 0, uid)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    e0 = rc.stats_errors(s.stats(), ref["st0"])
    s.step(True)
    e1 = rc.stats_errors(s.stats(), ref["st1"])
    gphi, gom, gU = s.get_state()
    tol = rc.stats_tol(precision, NY)
    print(f"STATS_ERR {precision} NX={NX} NY={NY} NZ={NZ}: prepare {max(e0):.3e} step {max(e1):.3e} "
          f"(rows {np.array2string(np.array(e0 + e1), precision=2)}) bound {tol:.1e}")
    # the step itself at the suite's tolerances (test_gpu_matches_oracle_large_ny), so that a
    # statistics error is not a state error in disguise
    tst, tU = (1e-9, 1e-11) if precision == "fp64" else (1e-4 * max(1.0, NY / 600), 1e-5)
    assert rel(gphi, ref["phi1"]) < tst and rel(gom, ref["om1"]) < tst and rel(gU, ref["U1"]) < tU
    assert max(e0) < tol, ("prepare()", e0)
    assert max(e1) < tol, ("step(True)", e1)
    assert s.health() == 0
    return s


@pytest.mark.parametrize("precision,NY", [("fp64", 33), ("fp64", 65), ("fp64", 129), ("fp64", 257), ("fp64", 385),
                                          ("fp32", 33), ("fp32", 65), ("fp32", 129), ("fp32", 257), ("fp32", 385),
                                          ("fp32", 633), ("fp32", 1201)])
def test_plane_stats_match_oracle(native, precision, NY):
    """One wave per line at R = 1, 2, 3, 5, 7 rows per lane (fp64 and fp32 storage) and the tall lines
    of NY = 633 and 1201 (fp32: LDS-staged tables, deferred slots) at NX = 16, NZ = 9."""
    check_stats(native, 16, NY, 9, precision)


def test_plane_stats_two_wave_lines(native, monkeypatch):
    """CHANNEL_KSPEC_HALVES=1: NY = 385 on two waves of R = 4 per line (the row map of the second half)."""
    monkeypatch.setenv("CHANNEL_KSPEC_HALVES", "1")
    check_stats(native, 16, 385, 9, "fp32")


def test_plane_stats_blocked_layout_padded_kz(native, monkeypatch):
    """CHANNEL_SPEC_KZB=1 at 32 x 33 x 17: nkz = 11 is no multiple of 8, so the blocked layout has
    padded kz lines, which must not count."""
    monkeypatch.setenv("CHANNEL_SPEC_KZB", "1")
    s = check_stats(native, 32, 33, 17, "fp64", seed=3, amp=0.3)
    assert s.spec_kzb() == 8 and s.plan.nkz % 8 != 0


def test_plane_stats_combine_mode(native, monkeypatch):
    """CHANNEL_COMBINE=1: K-SPEC writes D1 v, v, D1 omega; the statistics come from the same registers."""
    monkeypatch.setenv("CHANNEL_COMBINE", "1")
    s = check_stats(native, 16, 385, 9, "fp32")
    assert s.combine()


def test_plane_stats_kx_subblocks(native, monkeypatch):
    """The 1-rank RCCL communicator with CHANNEL_KBLOCKS=3: three K-SPEC launches accumulate into one
    statistics buffer, which then passes through the sum-allreduce."""
    monkeypatch.setenv("CHANNEL_KBLOCKS", "3")
    s = check_stats(native, 16, 129, 9, "fp64", uid=native.new_unique_id())
    assert s.kblocks() == 3 and s.comm_kind() == "rccl"
