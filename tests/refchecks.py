"""Shared references, bounds and preconditions of the time-step and plane-statistics tests
(test_timestep_gpu.py, test_statistics_gpu.py, test_multirank_gpu.py and the child scripts of
test_switches_gpu.py).  NumPy only: nothing here calls the native core."""
import math

import numpy as np

# CFL maxima against an fp64 reference.  The kernels convert |u|, |v|, |w| to fp32 and form the sum
# there.  fp64 storage: one fp64 -> fp32 conversion (2^-24 = 6e-8) on a plain maximum, three
# conversions, three products and two adds of non-negative fp32 terms (< 6 * 2^-24 = 3.6e-7) on the
# sum.  fp32 storage: the suite's bound on fp32 transform output.  Measured on the MI355X: fp64 <= 4.3e-8
# on a maximum, <= 4.6e-8 on the sum and on dt (kernel, solver paths and 2 .. 4 ranks alike); fp32
# <= 1.2e-7 at the kernel, <= 2.9e-7 on the solver's sum and dt.
TOL_MAX_F64, TOL_SUM_F64, TOL_CFL_F32 = 2e-7, 1e-6, 1e-4


def cfl_maxima(u, v, w, inv_dy_rows, cx, cz):
    """[|u|max, |v|max, |w|max, max(|u| cx + |v| / dy(y) + |w| cz)] of physical fields [ny, NX, Nz]."""
    u, v, w = np.abs(u), np.abs(v), np.abs(w)
    iy = np.asarray(inv_dy_rows)[:, None, None]
    return np.array([u.max(), v.max(), w.max(), (u * cx + v * iy + w * cz).max()])


def cfl_mutations(u, v, w, inv_dy, y0, cx, cz, chunk=0):
    """Relative change of the reference CFL sum under the mistakes the tests must catch: cx and cz
    swapped, inv_dy read without the plane offset (chunk = 0: inv_dy[y] for inv_dy[y0 + y]; chunk
    > 0: every `chunk` planes restart at row 0, the y-chunk pipeline's form of it), the v term
    dropped, the w term dropped and, for a plane range (chunk = 0), its rows reversed (a wrong row ->
    plane map)."""
    ny = u.shape[0]
    rows = inv_dy[y0:y0 + ny]
    s = cfl_maxima(u, v, w, rows, cx, cz)[3]
    nooff = inv_dy[np.arange(ny) % chunk] if chunk else inv_dy[:ny]
    z = np.zeros_like(u)
    mut = {
        "cx/cz swapped": cfl_maxima(u, v, w, rows, cz, cx)[3],
        "inv_dy without y0": cfl_maxima(u, v, w, nooff, cx, cz)[3],
        "v term dropped": cfl_maxima(u, z, w, rows, cx, cz)[3],
        "w term dropped": cfl_maxima(u, v, z, rows, cx, cz)[3],
    }
    if not chunk:  # (a whole grid's inv_dy is symmetric: reversing all NY planes shows nothing)
        mut["planes reversed"] = cfl_maxima(u, v, w, rows[::-1], cx, cz)[3]
    return {k: (m - s) / s for k, m in mut.items()}


def assert_cfl_sensitive(u, v, w, inv_dy, y0, cx, cz, chunk=0):
    """Precondition on the reference alone: every mutation moves the sum by >= 1e-3 relative, 1000
    times the fp64 tolerance (10 times the fp32 one)."""
    for name, d in cfl_mutations(u, v, w, inv_dy, y0, cx, cz, chunk).items():
        assert abs(d) >= 1e-3, f"the inputs cannot tell '{name}' from the right sum: moves it by {d:.2e}"


def dt_reference(maxima, cfl, dt_max, dt_fixed, parity, NX, NZ, LX, LZ, Re, NY):
    """(dt_c, dt_v, dt) of the time-step control, written from COMPAT.md A14 and the reference formula
    it cites (RK3.c:86-89).  Corrected mode: dt_c = cfl / max(|u| kx_max + |v| / dy + |w| kz_max),
    dt_max when that sum is not positive; the viscous terms are implicit, so no viscous limit.
    Parity mode: the reference's uniform dy = 2 / (NY - 1), its wavenumber factors NX / (2 pi L) (NX
    for the z term too) and its viscous limit cfl Re / (1 / dy^2 + (NX / 3 LX)^2 + (NZ / 3 LZ)^2)."""
    umax, vmax, wmax, csum = (float(x) for x in maxima)
    if parity:
        dy = 2.0 / (NY - 1)
        c = NX / (2 * math.pi * LX) * umax + vmax / dy + NX / (2 * math.pi * LZ) * wmax
        dt_c = cfl / c if c > 0 else dt_max
        dt_v = cfl * Re / (1.0 / dy ** 2 + (NX / (3.0 * LX)) ** 2 + (NZ / (3.0 * LZ)) ** 2)
    else:
        dt_c = cfl / csum if csum > 0 else dt_max
        dt_v = dt_max
    dt = min(dt_c, dt_v, dt_max)
    if dt_fixed > 0:
        dt = dt_fixed
    return dt_c, dt_v, dt


# ---- plane statistics ---------------------------------------------------------------------------
def stats_errors(got, ref):
    """Errors of the four rows <uu>, <vv>, <ww>, <uv> [4, NY] as vectors over y: uu, vv, ww relative
    to their own norm; uv, a signed sum, relative to the norm of sqrt(uu vv)."""
    got, ref = np.asarray(got).reshape(4, -1), np.asarray(ref)
    den = [np.linalg.norm(ref[0]), np.linalg.norm(ref[1]), np.linalg.norm(ref[2]),
           np.linalg.norm(np.sqrt(ref[0] * ref[1]))]
    return [np.linalg.norm(got[i] - ref[i]) / den[i] for i in range(4)]


# fp64: the y-line operators agree with the oracle to 1e-10 and the sums are quadratic.
# (measured on the MI355X, worst row: 1e-15 at NY = 33 to 8e-13 at NY = 385, every path alike).
# fp32 (the oracle gets the complex64-rounded state): 4 x the largest error measured over every
# fp32 case of the suite, rounded up to one digit, and never above twice the suite's fp32 state
# tolerance, 2e-4 max(1, NY / 600).  Measured on the MI355X, worst row (always vv or uv):
#   prepare(): 1e-15 .. 2e-11, the fp64 figures (the state is exact in fp32; K-SPEC works in fp64);
#              3e-8 through CHANNEL_KSPEC_SPLIT (the output kernel reads the stored fp32 v)
#   step(True), NX = 16, NZ = 9:  NY = 33 1.8e-7, 65 5.3e-7, 129 1.2e-6 (2.4e-6 after two steps),
#              257 7.7e-6, 385 5.7e-6 (two waves per line 5.7e-6, combine mode 5.5e-6, GLDS7 and
#              NS7=3 5.7e-6, split 6.6e-6; NY = 289 split 6.2e-6), 633 2.1e-5, 1201 3.15e-5
# largest 3.15e-5, times 4 = 1.26e-4, rounded up: 2e-4 (the cap below NY = 600, under it above).
STATS_TOL_F64 = 1e-9
STATS_TOL_F32 = 2e-4


def stats_tol(precision, NY):
    if precision == "fp64":
        return STATS_TOL_F64
    return min(STATS_TOL_F32, 2e-4 * max(1.0, NY / 600))


def oracle_stats_double_kz0(o):
    """<uu> of the oracle's prepared fields with the kz = 0 column counted twice (the -kz half of
    a column that has none): the mistake the uu comparison must see."""
    u = o.lines(o.fields[0])
    wgt = np.full(u.shape[1], 2.0)
    if o.mean_line is not None:
        wgt[o.mean_line] = 0
    return (np.abs(u) ** 2) @ wgt


def assert_stats_sensitive(o):
    """Preconditions on the reference alone (o.fields prepared): the kz = 0 weight matters to uu by
    >= 1e-2, and uv is not small against sqrt(uu vv) (>= 1e-2), so its relative bound is not vacuous.
    Holds on the rank that owns kz = 0; the full-spectrum oracle always does."""
    st = o.plane_stats()
    d = np.linalg.norm(oracle_stats_double_kz0(o) - st[0]) / np.linalg.norm(st[0])
    assert d >= 1e-2, f"double-counted kz = 0 moves uu by only {d:.2e}"
    r = np.linalg.norm(st[3]) / np.linalg.norm(np.sqrt(st[0] * st[1]))
    assert r >= 1e-2, f"|uv| is {r:.2e} of sqrt(uu vv)"
