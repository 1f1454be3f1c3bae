"""Restart onto another grid, host side: the interpolation table and the mode map of the C++ core
(regrid.hpp) and of the NumPy reference (reference/regrid.py), the preconditions of the GPU comparison
(test_regrid_gpu.py) and the config keys."""
import numpy as np
import pytest

import regridchecks as rc
from channel_gpu_amd.reference import regrid as rg


def numpy_table(NYs, ss, NYd, sd, width=6):
    return rg.interp_table(rg.tanh_grid(NYs, ss), rg.tanh_grid(NYd, sd), width)


def cpp_table(native, NYs, ss, NYd, sd):
    t = native.regrid_table(NYs, ss, NYd, sd)
    return np.asarray(t.j0), np.asarray(t.w)


TABLES = {"numpy": lambda native, *a: numpy_table(*a), "cpp": cpp_table}


def unit_rows(w):
    return int(np.sum((np.count_nonzero(w, axis=1) == 1) & (w.max(axis=1) == 1.0)))


@pytest.mark.parametrize("impl", sorted(TABLES))
@pytest.mark.parametrize("pair", [(33, 2.0, 49, 1.6), (49, 1.6, 33, 2.0)])
def test_polynomials_to_degree_five_are_exact(native, impl, pair):
    NYs, ss, NYd, sd = pair
    j0, w = TABLES[impl](native, *pair)
    ys, yd = rg.tanh_grid(NYs, ss), rg.tanh_grid(NYd, sd)
    for p in range(6):
        err = rc.maxerr(rg.apply_table(j0, w, ys ** p), yd ** p)
        assert err < 1e-13, (p, err)


@pytest.mark.parametrize("impl", sorted(TABLES))
def test_unit_rows_sums_and_lebesgue_bound(native, impl):
    table = TABLES[impl]
    _, w = table(native, 33, 2.0, 33, 2.0)
    assert unit_rows(w) == 33 and np.array_equal(w.sum(axis=1), np.ones(33))
    j0, w = table(native, 65, 2.0, 129, 2.0)
    assert unit_rows(w) == 65
    # the shared nodes are every second target node and they copy the source node j / 2
    for j in range(0, 129, 2):
        assert w[j, j // 2 - j0[j]] == 1.0
    worst = 0.0
    for pair in [(33, 2.0, 49, 1.6), (65, 2.0, 129, 2.0), (129, 2.0, 385, 2.0), (385, 2.0, 633, 2.0), (33, 2.0, 385, 2.0),
                 (49, 1.6, 33, 2.0), (33, 2.0, 33, 2.0)]:
        j0, w = table(native, *pair)
        for row in (0, -1):  # the walls copy the wall values
            assert np.count_nonzero(w[row]) == 1 and w[row].max() == 1.0
        assert j0[0] == 0 and np.argmax(w[0]) == 0 and j0[-1] + np.argmax(w[-1]) == pair[0] - 1
        assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-14, pair
        assert j0.min() >= 0 and (j0 + w.shape[1]).max() <= pair[0]
        worst = max(worst, np.abs(w).sum(axis=1).max())
    print(f"max sum |w| = {worst:.3f}")
    assert worst <= 3.0


@pytest.mark.parametrize("impl", sorted(TABLES))
def test_sixth_order(native, impl):
    f = lambda y: (1 - y ** 2) ** 2 * np.cos(3 * np.pi * y)  # noqa: E731
    yd = rg.tanh_grid(97, 1.6)
    err = {}
    for n in (65, 257):
        j0, w = TABLES[impl](native, n, 2.0, 97, 1.6)
        err[n] = rc.maxerr(rg.apply_table(j0, w, f(rg.tanh_grid(n, 2.0))), f(yd))
    print(f"err(65) = {err[65]:.3e}, err(257) = {err[257]:.3e}, ratio {err[65] / err[257]:.3e}")
    assert err[65] / err[257] >= 4 ** 5.5


@pytest.mark.parametrize("pair", [(33, 2.0, 49, 1.6), (49, 1.6, 33, 2.0), (65, 2.0, 129, 2.0), (33, 2.0, 33, 2.0),
                                  (129, 2.0, 385, 2.0), (1201, 2.0, 33, 2.0), (9, 2.0, 33, 2.0)])
def test_cpp_table_equals_numpy(native, pair):
    j0, w = numpy_table(*pair)
    t = native.regrid_table(*pair)
    assert np.array_equal(np.asarray(t.j0), j0)
    assert rc.maxerr(np.asarray(t.w), w) <= 1e-14
    # unit flags and the per-chunk source windows of the kernel
    unit = np.asarray(t.unit)
    for j in range(pair[2]):
        is_unit = np.count_nonzero(w[j]) == 1 and w[j].max() == 1.0
        assert (unit[j] >= 0) == is_unit and (not is_unit or w[j, unit[j]] == 1.0)
    win0, winlen = np.asarray(t.win0), np.asarray(t.winlen)
    assert len(win0) == (pair[2] + 7) // 8
    for c in range(len(win0)):
        rows = slice(8 * c, min(8 * c + 8, pair[2]))
        assert win0[c] == j0[rows].min() and win0[c] + winlen[c] == j0[rows].max() + t.W
    assert t.max_window() == winlen.max()


def test_widest_window_fits_the_lds_budget(native):
    """1536 -> 33 at stretch 2 reads the most source rows per 8 target planes of any pair the config
    admits: 342 rows, 8 lines of (342 | 1) fp64 complex = 43.9 KB of the kernel's 64 KB."""
    t = native.regrid_table(1536, 2.0, 33, 2.0)
    assert t.max_window() == 342
    assert 8 * (t.max_window() | 1) * 16 <= native.regrid_lds_bytes


@pytest.mark.parametrize("NXs,NXd", [(32, 48), (48, 32), (16, 32)])
@pytest.mark.parametrize("NZs,NZd", [(17, 25), (25, 17)])
def test_cpp_mode_map_equals_reference(native, NXs, NXd, NZs, NZd):
    planes, ntake = rg.plane_map(NXs, NXd), rg.mode_map(NXs, NZs, NXd, NZd)[1]
    nkx = 2 * (NXd // 3) + 1
    assert (planes >= 0).sum() == min(nkx, 2 * (NXs // 3) + 1)
    # both signs of kx map to the planes of the same |kx|
    Kd = NXd // 3
    for k in range(1, Kd + 1):
        assert (planes[k] >= 0) == (planes[nkx - k] >= 0) and (planes[k] < 0 or planes[nkx - k] == NXs - planes[k])
    start, count = [], []
    base, rem = divmod(nkx, 3)
    for r in range(3):
        count.append(base + (1 if r < rem else 0))
        start.append(sum(count[:r]))
    got = []
    for r in range(3):
        pl, nt = native.regrid_mode_map(NXs, NZs, NXd, NZd, start[r], count[r])
        assert nt == ntake
        got.append(np.asarray(pl))
    assert np.array_equal(np.concatenate(got), planes)
    whole, _ = native.regrid_mode_map(NXs, NZs, NXd, NZd, 0, nkx)
    assert np.array_equal(np.asarray(whole), planes)


def test_reference_modes_are_copied_or_zero():
    """x/z only (the same y grid): the retained band of the smaller grid is copied, the rest is zero."""
    phi, om, U = rc.source_state(rc.SMALL)
    gphi, gom, gU = rc.reference(rc.SMALL, rc.XZ)
    NY, nkx, nkz = rc.dims(rc.SMALL)
    Ks = rc.SMALL[0] // 3
    assert np.array_equal(gU, U)
    for f, g in ((phi, gphi), (om, gom)):
        assert np.array_equal(g[:, :Ks + 1, :nkz], f[:, :Ks + 1])
        assert np.array_equal(g[:, -Ks:, :nkz], f[:, -Ks:])
        assert not g[:, Ks + 1:-Ks].any() and not g[:, :, nkz:].any()
    # and back: truncation returns the source
    bphi, bom, bU = rg.regrid_state(gphi, gom, gU, src=rc.XZ, dst=rc.SMALL)
    assert np.array_equal(bphi, phi) and np.array_equal(bom, om) and np.array_equal(bU, U)


def test_gpu_bound_tells_the_stencil_width():
    """Precondition of the y comparison on the GPU (test_regrid_gpu.py: every field of the regridded state
    within 1e-12 of its maximum in fp64, 2e-7 with fp32 storage): for random_state(seed=5, amp=0.3) on
    32x33x17 -> 49 points at stretch 1.6, a 4-point interpolation lies at least 0.1 and a linear one at least
    0.2 of the field maximum away from the 6-point reference, so an implementation with a narrower stencil
    cannot pass that comparison.

    One figure per variant, as the GPU comparison needs it: the state fails the comparison as soon as one
    of its fields does, so the figure is the largest, over phi and omega, of max|variant - reference| /
    max|reference| of that field.  Measured: 0.122 (4-point) and 0.269 (linear), both set by phi.  Per
    field: phi 0.122 and 0.269, omega 0.073 and 0.216 (omega is (1 - y^2) times node-wise noise; phi =
    D2 v - k^2 v of such noise is rougher, so its variants lie further apart).  omega alone would miss the
    0.1 for the 4-point variant.  Each field on its own must still be far outside both GPU bounds: at
    least 1e-3 of its maximum, four orders above the wider bound, 2e-7."""
    ref = rc.reference(rc.SMALL, rc.FINE, 6)
    figure = {}
    for name, width in (("4-point", 4), ("linear", 2)):
        var = rc.reference(rc.SMALL, rc.FINE, width)
        per_field = [rc.maxerr(var[k], ref[k]) / np.abs(ref[k]).max() for k in range(2)]
        print(f"{name}: phi {per_field[0]:.3f}, omega {per_field[1]:.3f} of the field maximum")
        assert min(per_field) >= 1e-3, (name, per_field)
        figure[name] = max(per_field)
    assert figure["4-point"] >= 0.1
    assert figure["linear"] >= 0.2


def test_config_keys_round_trip(native):
    c = native.Config()
    assert c.regrid is False and c.regrid_stretch == 0.0
    c = native.Config.from_string("NX = 32; NY = 33; NZ = 17; regrid = true; regrid_stretch = 1.6;")
    assert c.regrid is True and c.regrid_stretch == 1.6
    c2 = native.Config.from_string(c.to_string())
    assert c2.regrid is True and c2.regrid_stretch == 1.6
    c3 = native.Config.from_string(native.Config().to_string())
    assert c3.regrid is False and c3.regrid_stretch == 0.0
    with pytest.raises(RuntimeError, match="regrid_stretch"):
        native.Config.from_string("NX = 32; NY = 33; NZ = 17; regrid_stretch = -1.0;")
