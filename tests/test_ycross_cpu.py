"""Cross-spectra of every plane against reference planes on the CPU: the reference
(reference/cross_spectra.py) against directly computed circular cross-correlations of the oracle's
physical fields, its identities (y = y_r against the plane spectra, the swap of two reference planes,
the parities under the reflection of the flow), the config keys and the folding of
TurbulenceStatistics.cross_correlations.  Tolerance 1e-12 of a row's maximum, as test_yspectra_cpu.py."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import TurbulenceStatistics
from channel_gpu_amd.reference import cross_spectra as xsp
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import spectra as spc

NX, NY, NZ = 16, 17, 9
REFS = [0, 3, 8, 12, 16]
SETS = ("velocity", "shear")


@functools.lru_cache(maxsize=None)
def _case():
    """Oracle state, its cross-spectra of both row sets, its plane spectra and the fluctuating physical
    fields [6, NY, NX, Nzp]; computed once, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    cs = {rows: xsp.plane_cross_spectra(o, REFS, rows) for rows in SETS}
    sp = spc.plane_spectra(o)
    ph = ora.spec_to_phys_full(o.fields, o.plan)
    ph = ph - ph.mean(axis=(2, 3), keepdims=True)
    for a in [ph, sp["ekx"], sp["ekz"]] + [c[k] for c in cs.values() for k in ("ckx", "ckz")]:
        a.setflags(write=False)
    return o, cs, sp, ph


def _direct(ph, fa, fb, yr, axis, n):
    """<a'(x + r, y, z) b'(x, y_r, z)> at r = -n/2 .. n/2 - 1 for every y: [NY, n]."""
    a, b = ph[fa], ph[fb][yr]
    return np.stack([(np.roll(a, -r, axis=1 + axis) * b).mean(axis=(1, 2)) for r in np.arange(n) - n // 2], axis=1)


def test_rows_and_shapes():
    o, cs, _, _ = _case()
    assert cs["velocity"]["rows"] == ("uu", "vv", "ww", "uv") and cs["shear"]["rows"] == ("u_wz", "v_wz", "w_wx", "wz_wz")
    for rows in SETS:
        c = cs[rows]
        assert c["ref_planes"] == REFS
        assert c["ckx"].shape == (4, len(REFS), NY, o.plan.Kx + 1) and c["ckz"].shape == (4, len(REFS), NY, o.plan.nkz)
        assert c["ckx"].dtype == c["ckz"].dtype == np.complex128
        # bin 0 of ckx keeps the real part only
        assert not c["ckx"][..., 0].imag.any()
    for bad in ([], [3, 3], [-1], [NY], list(range(17))):
        with pytest.raises(ValueError):
            xsp.plane_cross_spectra(o, bad)
    with pytest.raises(ValueError):
        xsp.plane_cross_spectra(o, [3], "pressure")
    with pytest.raises(ValueError):
        xsp.cross_correlations(np.ones(6), 8)


@pytest.mark.parametrize("axis", ["x", "z"])
@pytest.mark.parametrize("rows", SETS)
def test_against_direct_cross_correlations(rows, axis):
    o, cs, _, ph = _case()
    ax_, n, c = (0, NX, cs[rows]["ckx"]) if axis == "x" else (1, o.plan.Nzp, cs[rows]["ckz"])
    got = xsp.cross_correlations(c, n)
    assert got.shape == (4, len(REFS), NY, n)
    for q, (name, fa, fb) in enumerate(xsp.CROSS_ROWS[rows]):
        want = np.stack([_direct(ph, fa, fb, yr, ax_, n) for yr in REFS])
        scale = np.abs(want).max()
        assert scale > 0
        err = np.abs(got[q] - want).max() / scale
        print(f"{rows} {name} R_{axis}: rel. error {err:.2e}")
        assert err < 1e-12, (rows, name, axis)
        # the sum of the real parts over the bins is the covariance at zero separation
        assert np.abs(c[q].real.sum(-1) - want[:, :, n // 2]).max() < 1e-12 * scale


def test_equal_planes_are_the_plane_spectra():
    _, cs, sp, _ = _case()
    for e, k in (("ekx", "ckx"), ("ekz", "ckz")):
        for q in range(4):
            got = np.stack([cs["velocity"][k][q, i, yr] for i, yr in enumerate(REFS)])
            assert np.abs(got.real - sp[e][q][REFS]).max() < 1e-12 * np.abs(sp[e][q]).max(), (e, q)
            if q < 3:
                assert np.abs(got.imag).max() < 1e-12 * np.abs(sp[e][q]).max(), (e, q)
        got = np.stack([cs["shear"][k][3, i, yr] for i, yr in enumerate(REFS)])
        assert np.abs(got - sp[e][6][REFS]).max() < 1e-12 * np.abs(sp[e][6]).max(), e


def test_swap_of_reference_planes():
    """Auto rows: the plane and the reference plane exchanged is the conjugate."""
    _, cs, _, _ = _case()
    for rows, autos in (("velocity", (0, 1, 2)), ("shear", (3,))):
        for k in ("ckx", "ckz"):
            c = cs[rows][k]
            for q in autos:
                for i, yi in enumerate(REFS):
                    for j, yj in enumerate(REFS):
                        assert np.abs(c[q, i, yj] - np.conj(c[q, j, yi])).max() <= 1e-12 * np.abs(c[q]).max(), (rows, k, q, i, j)


def test_maps_are_not_symmetric_in_rx():
    """Away from the reference plane the imaginary parts carry the inclination of the structures: the
    maps differ between +r_x and -r_x.  Fails if the imaginary parts are lost or the wrong side is
    conjugated (the direct check above), here without the physical fields."""
    _, cs, _, _ = _case()
    c = cs["velocity"]["ckx"]
    i = REFS.index(3)
    for q in (0, 2):  # uu, ww
        assert np.abs(c[q, i].imag).max() > 0.1 * np.abs(c[q, i]).max()
        R = xsp.cross_correlations(c[q, i], NX)          # [NY, NX], r = -NX/2 .. NX/2 - 1
        pos, neg = R[:, NX // 2 + 1:], R[:, NX // 2 - 1:0:-1]
        assert np.abs(pos - neg).max() > 0.1 * np.abs(R).max()
        # at the reference plane itself an auto-correlation is symmetric
        assert np.abs(pos[3] - neg[3]).max() < 1e-12 * np.abs(R).max()


def test_parities_of_the_reflected_flow():
    """The reflection y -> -y of the flow (v -> -v: phi(y) -> -phi(-y), omega_y(y) -> omega_y(-y)):
    every row is mirrored in y and in the reference plane, uv, u_wz and w_wx with the opposite sign, the
    parities the fold assumes.  The two states go through different floating-point solves; 1e-9."""
    o, cs, _, _ = _case()
    m = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=400.0)
    m.set_state(-o.phi[::-1], o.om[::-1], o.U[::-1])
    m.prepare()
    for rows in SETS:
        cm = xsp.plane_cross_spectra(m, [NY - 1 - j for j in REFS], rows)
        for k in ("ckx", "ckz"):
            for q, name in enumerate(cm["rows"]):
                sgn = -1.0 if name in xsp.ODD_ROWS else 1.0
                err = np.abs(cm[k][q][:, ::-1] - sgn * cs[rows][k][q]).max() / np.abs(cs[rows][k][q]).max()
                assert err < 1e-9, (rows, k, name, err)
    assert set(xsp.ODD_ROWS) == {"uv", "u_wz", "w_wx"}


def _stats(samples, rows, refs, nu=1.0 / 180.0, ut=(0.06, 0.07)):
    """samples: (ckx, ckz, ekx, ekz) per sample."""
    o = _case()[0]
    S = TurbulenceStatistics(o.ops.y, nu)
    kx, kz = o.plan.ax * np.arange(o.plan.Kx + 1), o.plan.az * np.arange(o.plan.nkz)
    for ckx, ckz, ekx, ekz in samples:
        S.add(o.U, o.plane_stats().ravel(), ut[0], ut[1], 0.0)
        S.add_cross_spectra(ckx, ckz, refs, xsp.row_names(rows), ekx, ekz, kx, kz, NX, o.plan.Nzp)
    return S


@pytest.mark.parametrize("rows", SETS)
def test_cross_correlations_of_the_statistics(rows):
    o, cs, sp, _ = _case()
    c = cs[rows]
    nu, ut = 1.0 / 180.0, np.sqrt(0.5 * (0.06 ** 2 + 0.07 ** 2))
    sel = [REFS.index(3), REFS.index(8)]  # (no mirror pair: nothing is folded)
    S = _stats([(c["ckx"][:, sel], c["ckz"][:, sel], sp["ekx"], sp["ekz"])] * 2, rows, [3, 8])
    assert S.ncs == 2
    r = S.cross_correlations()
    Nzp = o.plan.Nzp
    assert list(r["ref_planes"]) == [3, 8]
    assert np.allclose(r["y_plus"], (1 + o.ops.y) * ut / nu, rtol=1e-13) and np.allclose(r["ref_y_plus"], r["y_plus"][[3, 8]], rtol=1e-13)
    assert np.allclose(r["r_x_plus"], (np.arange(NX) - NX // 2) * (2 * np.pi / NX) * ut / nu, rtol=1e-13)
    assert np.allclose(r["r_z_plus"], (np.arange(Nzp) - Nzp // 2) * (np.pi / Nzp) * ut / nu, rtol=1e-13)
    row_of = {name: q for q, name in enumerate(spc.SPECTRA_ROWS)}
    for q, name in enumerate(c["rows"]):
        fa, fb = xsp.ROW_FACTORS[name]
        va, vb = sp["ekx"][row_of[fa]].sum(-1), sp["ekx"][row_of[fb]].sum(-1)
        for key, k, n in (("x", "ckx", NX), ("z", "ckz", Nzp)):
            R = r["R_" + key][name]
            assert R.shape == (2, NY, n) and np.isfinite(R).all() and np.abs(R).max() <= 1 + 1e-12
            den = np.sqrt(va[None, :] * vb[[3, 8]][:, None])
            want = xsp.cross_correlations(c[k][q][sel], n) / np.where(den > 0, den, np.inf)[:, :, None]
            assert np.abs(R - want).max() < 1e-12, (name, key)
            coh = r["coherence_k" + key][name]
            assert coh.shape == c[k][q][sel].shape and np.isfinite(coh).all() and coh.min() >= 0
        Ry = r["R_y"][name]
        assert Ry.shape == (2, NY) and np.abs(Ry - r["R_x"][name][:, :, NX // 2]).max() < 1e-12
        if fa == fb:
            assert abs(Ry[0, 3] - 1) < 1e-12 and abs(Ry[1, 8] - 1) < 1e-12
            # (an auto row at its own plane is fully coherent in every non-empty bin)
            assert np.abs(r["coherence_kz"][name][0, 3][sp["ekz"][row_of[fa]][3] > 0] - 1).max() < 1e-12
    with pytest.raises(ValueError):
        TurbulenceStatistics(o.ops.y, nu).cross_correlations()
    with pytest.raises(ValueError):
        S.add_cross_spectra(c["ckx"], c["ckz"], REFS, c["rows"], sp["ekx"], sp["ekz"], r["r_x_plus"], r["r_z_plus"])


@pytest.mark.parametrize("rows", SETS)
def test_folding_of_a_mirrored_state(rows):
    """The state and its mirror image in y (the arrays flipped in y and in the reference plane), sampled
    at a plane and its mirror: the antisymmetric rows cancel exactly, the symmetric rows are those of the
    state alone."""
    _, cs, sp, _ = _case()
    c = cs[rows]
    refs = [3, NY - 1 - 3]
    full = xsp.plane_cross_spectra(_case()[0], refs, rows)
    a = (full["ckx"], full["ckz"], sp["ekx"], sp["ekz"])
    b = (full["ckx"][:, ::-1, ::-1], full["ckz"][:, ::-1, ::-1], sp["ekx"][:, ::-1], sp["ekz"][:, ::-1])
    one = _stats([a], rows, refs).cross_correlations()
    both = _stats([a, b], rows, refs).cross_correlations()
    assert list(one["ref_planes"]) == [3] and list(both["ref_planes"]) == [3]
    for name in c["rows"]:
        for key in ("R_x", "R_z", "R_y", "coherence_kx", "coherence_kz"):
            assert one[key][name].shape[0] == 1
            if name in xsp.ODD_ROWS:
                assert np.array_equal(both[key][name], np.zeros_like(both[key][name])), (name, key)
                assert np.abs(one[key][name]).max() > 0
            else:
                assert np.abs(both[key][name] - one[key][name]).max() <= 1e-13 * np.abs(one[key][name]).max(), (name, key)
    # a single plane stands alone
    alone = _stats([(full["ckx"][:, :1], full["ckz"][:, :1], sp["ekx"], sp["ekz"])], rows, [3]).cross_correlations()
    den = np.sqrt(sp["ekx"][0].sum(-1) * sp["ekx"][0 if rows == "velocity" else 6].sum(-1)[3])
    want = xsp.cross_correlations(full["ckx"][0, 0], NX) / np.where(den > 0, den, np.inf)[:, None]
    assert np.abs(alone["R_x"][c["rows"][0]][0] - want).max() < 1e-12


def test_config_keys():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    d = C.Config()
    assert d.ycross_every == 0 and d.ycross_planes == "" and d.ycross_rows == "velocity"
    c = default_config(NX=32, NY=33, NZ=17, ycross_every=6, ycross_planes="0, 7,32", ycross_rows="shear")
    s = c.to_string()
    assert "ycross_every = 6;" in s and 'ycross_planes = "0, 7,32";' in s and 'ycross_rows = "shear";' in s
    back = C.Config.from_string(s)
    assert back.ycross_every == 6 and back.ycross_planes == "0, 7,32" and back.ycross_rows == "shear"
    e = C.Config.from_string('NX = 32; NY = 33; NZ = 17; ycross_every = 3; ycross_planes = "5";')
    assert e.ycross_every == 3 and e.ycross_rows == "velocity"
    # planes alone are accepted (the key is off), but checked
    default_config(NX=32, NY=33, NZ=17, ycross_planes="1,2")
    for bad in (dict(ycross_every=-1), dict(ycross_every=2), dict(ycross_every=2, ycross_planes=""),
                dict(ycross_every=2, ycross_planes="3,3"), dict(ycross_every=2, ycross_planes="33"),
                dict(ycross_every=2, ycross_planes="-1"), dict(ycross_every=2, ycross_planes="a"),
                dict(ycross_every=2, ycross_planes=",".join(map(str, range(17)))),
                dict(ycross_every=2, ycross_planes="3", ycross_rows="pressure"), dict(ycross_planes="3,3")):
        with pytest.raises(RuntimeError):
            default_config(NX=32, NY=33, NZ=17, **bad)
