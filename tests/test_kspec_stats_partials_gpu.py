"""K-SPEC's plane statistics as per-workgroup partial sums (SpecArgs::stats_part) and their
fixed-order reduction (kspec_stats_reduce), on grids where the tiles of lines exceed the resident
grid, so that a workgroup accumulates several tiles into its row of partials: what the cases of
test_statistics_gpu.py (NX = 16, NZ = 9: a few dozen tiles, at most one per workgroup) never do.

Compared with the NumPy oracle's plane_stats() as test_statistics_gpu.check_stats does
(refchecks.stats_errors against refchecks.stats_tol).  No case asserts bitwise run-to-run equality:
the sum over the lines of a tile still uses LDS atomics, whose order is free."""
import functools

import numpy as np
import pytest

import refchecks as rc
import test_statistics_gpu as tsg
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config

pytestmark = pytest.mark.gpu

# case 2's grid: nkx = 85, nkz = 43: 3,655 lines, lines % 4 = 3 (a partial last tile), R = 3
G2 = (128, 129, 65)


@functools.lru_cache(maxsize=None)
def prepared_reference(NX, NY, NZ, precision, seed=5, amp=0.05):
    """The oracle's statistics of the standard random state (fp32: rounded through complex64), no
    step: computed once per grid and precision and shared read-only."""
    o = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=tsg.DT)
    phi, om = ora.random_state(o.plan, o.ops, seed=seed, amp=amp)
    if precision == "fp32":
        phi = phi.astype(np.complex64).astype(np.complex128)
        om = om.astype(np.complex64).astype(np.complex128)
    U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
    o.set_state(phi, om, U)
    o.prepare()
    rc.assert_stats_sensitive(o)
    out = dict(phi=phi, om=om, U=U, st0=o.plane_stats())
    for a in out.values():
        a.setflags(write=False)
    return out


def stats_solver(native, NX, NY, NZ, precision, uid=b""):
    cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision=precision, dt_fixed=tsg.DT, stats_every=1, log_every=0,
                         symmetry_every=0, ic="zero")
    return native.Solver(cfg, 0, 1, 0, uid)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_prepare_r7_blocked_several_tiles_per_workgroup(native, precision):
    """96 x 385 x 49, blocked layout: nkx = 65, nkz = 33 padded to 40, 2,600 lines = 650 tiles of 4
    for at most 256 resident workgroups (2.5 rounds, the last one partial), NY = 385 < 64 * 7 rows.
    prepare() only (K-SPEC mode 0 with statistics)."""
    NX, NY, NZ = 96, 385, 49
    ref = prepared_reference(NX, NY, NZ, precision)
    s = stats_solver(native, NX, NY, NZ, precision)
    assert s.spec_kzb() == 8 and s.plan.nkz % 8 != 0
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    e0 = rc.stats_errors(s.stats(), ref["st0"])
    tol = rc.stats_tol(precision, NY)
    print(f"STATS_ERR {precision} {NX}x{NY}x{NZ} prepare: rows {np.array2string(np.array(e0), precision=2)} bound {tol:.1e}")
    assert native.kspec_last_variant().startswith("kspec_kernel<7, "), native.kspec_last_variant()
    assert max(e0) < tol, ("prepare()", e0)
    assert s.health() == 0


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_prepare_and_step_r3_partial_last_tile(native, precision):
    """128 x 129 x 65 (R = 3): 3,655 lines, lines % 4 = 3.  prepare() and step(True) against the
    oracle, and the stepped state at the suite's tolerances (check_stats)."""
    tsg.check_stats(native, *G2, precision)


def test_kx_subblock_launches_accumulate(native, monkeypatch):
    """The 1-rank RCCL communicator with CHANNEL_KBLOCKS=3 on case 2's grid: three K-SPEC launches
    add to the same partials before the one reduction (then the sum-allreduce)."""
    monkeypatch.setenv("CHANNEL_KBLOCKS", "3")
    s = tsg.check_stats(native, *G2, "fp64", uid=native.new_unique_id())
    assert s.kblocks() == 3 and s.comm_kind() == "rccl"


def test_no_stale_partials_between_statistics_steps(native):
    """step(True) three times on one solver with plain steps between (the step graphs replayed): each
    stats() is the statistics of that state, not a running sum: it equals a fresh solver's
    prepare() statistics of the same state to stats_tol."""
    ref = tsg.reference(*G2, "fp64")
    s = stats_solver(native, *G2, "fp64")
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    tol = rc.stats_tol("fp64", G2[1])
    got = []
    for plain in (0, 2, 1):
        for _ in range(plain):
            s.step(False)
        s.step(True)
        got.append((np.asarray(s.stats()).reshape(4, -1).copy(), s.get_state()))
    assert s.graph_active()
    e1 = rc.stats_errors(got[0][0], ref["st1"])
    assert max(e1) < tol, ("first step(True) against the oracle", e1)
    for k, (st, state) in enumerate(got):
        f = stats_solver(native, *G2, "fp64")
        f.set_state(*state)
        f.prepare()
        e = rc.stats_errors(st, np.asarray(f.stats()).reshape(4, -1))
        print(f"statistics step {k}: against a fresh solver's prepare() {np.array2string(np.array(e), precision=2)} bound {tol:.1e}")
        assert max(e) < tol, (k, e)
    # (the states differ, so do their statistics: the comparison above is not one of equal things)
    assert not np.array_equal(got[0][0], got[2][0])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_second_moments_agree_with_plane_moments(native, precision):
    """Sanity row: the physical-space second moments of Solver.plane_moments() against K-SPEC's
    Parseval sums of the same prepared state, per row relative to the row's maximum, at
    test_physfields_gpu.test_moments' tolerance for these rows (1e-10 in fp64, 1e-5 in fp32)."""
    ref = tsg.reference(*G2, precision)
    s = stats_solver(native, *G2, precision)
    s.set_state(ref["phi"], ref["om"], ref["U"])
    s.prepare()
    m = s.plane_moments()
    st = np.asarray(s.stats()).reshape(4, G2[1])
    tol = 1e-10 if precision == "fp64" else 1e-5
    for r in range(4):
        err = np.abs(m[1 + r] - st[r]).max() / np.abs(st[r]).max()
        print(f"moment row {1 + r} vs K-SPEC stats: rel. error {err:.3e} (tol {tol:.1e})")
        assert err < tol
