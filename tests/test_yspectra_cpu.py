"""One-dimensional spectra at every plane on the CPU: the reference (reference/spectra.py) against
independent physical-space evaluations, Parseval against the plane statistics, the two-point
correlations against direct circular correlations, and the wall-unit spectra of TurbulenceStatistics."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.models.statistics import SPECTRA_ROWS, TurbulenceStatistics
from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import spectra as spc

NX, NY, NZ = 16, 17, 9
# (row, first field, second field) of the physical fields u, v, w, wx, wy, wz, p
PAIRS = (("uu", 0, 0), ("vv", 1, 1), ("ww", 2, 2), ("uv", 0, 1), ("wxwx", 3, 3), ("wywy", 4, 4), ("wzwz", 5, 5), ("pp", 6, 6))


@functools.lru_cache(maxsize=None)
def _case():
    """Oracle state, a band-limited real 'pressure' (a combination of its fields), the reference
    spectra and the fluctuating physical fields [7, NY, NX, Nzp]; computed once, read-only."""
    o = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=400.0)
    phi, om = ora.random_state(o.plan, o.ops, seed=9, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    o.prepare()
    p_hat = 0.5 * o.fields[1] + 0.25 * o.fields[4]
    p_hat[:, 0, 0] = 0
    sp = spc.plane_spectra(o, p_hat)
    ph = ora.spec_to_phys_full(np.concatenate([o.fields, p_hat[None]]), o.plan)
    ph = ph - ph.mean(axis=(2, 3), keepdims=True)
    for a in (sp["ekx"], sp["ekz"], ph):
        a.setflags(write=False)
    return o, p_hat, sp, ph


def _check(got, ref, tol, what):
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{what}: rel. error {err:.2e} (tol {tol:.0e})")
    assert err < tol, what


def test_rows_and_shapes():
    o, _, sp, _ = _case()
    assert tuple(sp["rows"]) == SPECTRA_ROWS == spc.SPECTRA_ROWS and len(SPECTRA_ROWS) == 8
    assert sp["ekx"].shape == (8, NY, o.plan.Kx + 1) and sp["ekz"].shape == (8, NY, o.plan.nkz)
    assert np.array_equal(spc.plane_spectra(o)["ekx"][7], np.zeros((NY, o.plan.Kx + 1)))


def test_ekx_against_physical_space():
    """FFT along x of the fluctuations, the mean over z of Re(a b*), +kx and -kx folded."""
    o, _, sp, ph = _case()
    K = o.plan.Kx
    F = np.fft.fft(ph, axis=2, norm="forward")
    for r, (name, i, j) in enumerate(PAIRS):
        full = (F[i] * np.conj(F[j])).real.mean(axis=2)  # [NY, NX]
        ref = np.zeros((NY, K + 1))
        ref[:, 0] = full[:, 0]
        ref[:, 1:] = full[:, 1:K + 1] + full[:, :-K - 1:-1]
        # (nothing above the retained band)
        assert np.abs(full[:, K + 1:NX - K]).max() <= 1e-14 * np.abs(full).max()
        _check(sp["ekx"][r], ref, 1e-12, f"ekx {name}")


def test_ekz_against_physical_space():
    """Real FFT along z, the mean over x of Re(a b*), kz > 0 counted twice."""
    o, _, sp, ph = _case()
    nkz = o.plan.nkz
    F = np.fft.rfft(ph, axis=3, norm="forward")
    wgt = np.where(np.arange(F.shape[3]) == 0, 1.0, 2.0)
    for r, (name, i, j) in enumerate(PAIRS):
        full = (F[i] * np.conj(F[j])).real.mean(axis=1) * wgt  # [NY, NZ]
        assert np.abs(full[:, nkz:]).max() <= 1e-14 * np.abs(full).max()
        _check(sp["ekz"][r], full[:, :nkz], 1e-12, f"ekz {name}")


def test_parseval():
    o, p_hat, sp, ph = _case()
    st, g = o.plane_stats(), bud.gradient_sums(o)
    for e in ("ekx", "ekz"):
        s = sp[e].sum(axis=-1)
        for r in range(4):
            _check(s[r], st[r], 1e-12, f"{e} row {SPECTRA_ROWS[r]} against plane_stats")
        for r in range(3):
            _check(s[4 + r], g[r], 1e-12, f"{e} row {SPECTRA_ROWS[4 + r]} against gradient_sums")
        _check(s[7], (ph[6] ** 2).mean(axis=(1, 2)), 1e-12, f"{e} row pp against the plane mean")


@pytest.mark.parametrize("axis", ["x", "z"])
def test_correlations_against_direct(axis):
    """The cosine transform of the uu spectrum equals the circular two-point correlation of u'."""
    o, _, sp, ph = _case()
    j = 5
    u = ph[0][j]
    ax_, n, e = (0, NX, sp["ekx"][0, j]) if axis == "x" else (1, o.plan.Nzp, sp["ekz"][0, j])
    direct = np.array([(u * np.roll(u, -r, axis=ax_)).mean() for r in range(n // 2 + 1)])
    direct /= direct[0]
    got = spc.correlations(e, n)
    assert got.shape == (n // 2 + 1,) and got[0] == 1.0
    assert np.abs(got - direct).max() < 1e-12
    # every plane at once; a zero spectrum (the walls of a no-slip flow) gives 0
    allp = spc.correlations(sp["ekx"][0], NX)
    assert allp.shape == (NY, NX // 2 + 1)
    assert np.abs(allp[j] - spc.correlations(sp["ekx"][0, j], NX)).max() < 1e-15
    assert np.array_equal(spc.correlations(np.zeros((2, 5)), 8), np.zeros((2, 5)))
    with pytest.raises(ValueError):
        spc.correlations(np.ones(6), 8)


def _stats(samples, ut=(0.06, 0.07), nu=1.0 / 180.0, **kw):
    o = _case()[0]
    S = TurbulenceStatistics(o.ops.y, nu)
    kx, kz = o.plan.ax * np.arange(o.plan.Kx + 1), o.plan.az * np.arange(o.plan.nkz)
    for ekx, ekz in samples:
        S.add(o.U, o.plane_stats().ravel(), ut[0], ut[1], 0.0)
        S.add_spectra(ekx, ekz, kx, kz, **kw)
    return S, kx, kz


def test_folding_of_a_mirrored_state():
    """The state and its mirror image in y (the arrays flipped): the antisymmetric fold of uv cancels
    exactly, the symmetric fold of uu is that of the state alone."""
    _, _, sp, _ = _case()
    one = _stats([(sp["ekx"], sp["ekz"])])[0].spectra()
    both = _stats([(sp["ekx"], sp["ekz"]), (sp["ekx"][:, ::-1], sp["ekz"][:, ::-1])])[0].spectra()
    h = (NY + 1) // 2
    for e in ("E_kx", "E_kz"):
        assert both[e]["uv"].shape == (h, sp["ekx" if e == "E_kx" else "ekz"].shape[2])
        assert np.array_equal(both[e]["uv"], np.zeros_like(both[e]["uv"]))
        assert np.abs(one[e]["uv"]).max() > 0
        assert np.abs(both[e]["uu"] - one[e]["uu"]).max() <= 1e-14 * one[e]["uu"].max()


def test_reflected_flow_has_mirrored_spectra():
    """The reflection y -> -y of the flow (v -> -v: phi(y) -> -phi(-y), omega_y(y) -> omega_y(-y), U
    even): every auto-spectrum is mirrored and the co-spectrum uv mirrored with the opposite sign, the
    parities the fold assumes.  The two states go through different floating-point solves; 1e-9."""
    o, _, sp, _ = _case()
    m = ora.OracleSolver(NX=NX, NY=NY, NZ=NZ, Re=400.0)
    m.set_state(-o.phi[::-1], o.om[::-1], o.U[::-1])
    m.prepare()
    sm = spc.plane_spectra(m)
    for e in ("ekx", "ekz"):
        for r in range(7):
            sgn = -1.0 if SPECTRA_ROWS[r] == "uv" else 1.0
            _check(sm[e][r], sgn * sp[e][r][::-1], 1e-9, f"{e} row {SPECTRA_ROWS[r]} of the reflected flow")


def test_wall_units():
    o, _, sp, _ = _case()
    nu, ut_lo, ut_hi = 1.0 / 180.0, 0.06, 0.07
    S, kx, kz = _stats([(sp["ekx"], sp["ekz"]), (2.0 * sp["ekx"], 2.0 * sp["ekz"])], (ut_lo, ut_hi), nu, nx=NX, nz=o.plan.Nzp)
    assert S.nsp == 2
    r = S.spectra()
    ut = np.sqrt(0.5 * (ut_lo ** 2 + ut_hi ** 2))
    h = (NY + 1) // 2
    lo, hi = np.arange(h), NY - 1 - np.arange(h)
    close = lambda a, b: np.abs(a - b).max() <= 1e-13 * np.abs(b).max()  # noqa: E731
    assert close(r["y_plus"], (1 + o.ops.y[lo]) * ut / nu)
    assert close(r["kx_plus"], kx * nu / ut) and close(r["kz_plus"], kz * nu / ut)
    assert np.isinf(r["lambda_x_plus"][0]) and close(r["lambda_z_plus"][1:], 2 * np.pi * ut / nu / kz[1:])
    unit = {"uu": ut ** 2, "vv": ut ** 2, "ww": ut ** 2, "uv": ut ** 2, "wxwx": ut ** 4 / nu ** 2, "wywy": ut ** 4 / nu ** 2,
            "wzwz": ut ** 4 / nu ** 2, "pp": ut ** 4}
    for e, k, key, n, dx in (("ekx", kx, "x", NX, 2 * np.pi / NX), ("ekz", kz, "z", o.plan.Nzp, np.pi / o.plan.Nzp)):
        for q, row in enumerate(SPECTRA_ROWS):
            a = 1.5 * sp[e][q]  # (the mean of the two samples)
            want = 0.5 * (a[lo] + (-1.0 if row == "uv" else 1.0) * a[hi]) / unit[row]
            assert close(r["E_k" + key][row], want), (e, row)
            # k Phi(k) with Phi = E / dk: the area under it over log k is the energy
            assert close(r["premult_k" + key][row], k / k[1] * want), (e, row)
            if row == "uv":
                assert row not in r["R_" + key]
            else:
                assert close(r["R_" + key][row], spc.correlations(want, n)), (e, row)
                assert r["R_" + key][row].shape == (h, n // 2 + 1)
        assert close(r[f"r_{key}_plus"], np.arange(n // 2 + 1) * dx * ut / nu)
    # the sum over k of the wall-unit spectrum is the folded mean square of profiles()
    p = S.profiles()
    assert np.abs(np.sqrt(r["E_kx"]["uu"].sum(axis=1) / 1.5) - p["urms"]).max() < 1e-12 * p["urms"].max()
    with pytest.raises(ValueError):
        TurbulenceStatistics(o.ops.y, nu).spectra()
    with pytest.raises(ValueError):
        S.add_spectra(sp["ekx"][:7], sp["ekz"][:7], kx, kz)


def test_config_keys():
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    assert C.Config().yspectra_every == 0 and C.Config().yspectra_pressure == 0
    c = default_config(NX=32, NY=33, NZ=17, yspectra_every=6, yspectra_pressure=1)
    assert "yspectra_every = 6;" in c.to_string() and "yspectra_pressure = 1;" in c.to_string()
    back = C.Config.from_string(c.to_string())
    assert back.yspectra_every == 6 and back.yspectra_pressure == 1
    d = C.Config.from_string("NX = 32; NY = 33; NZ = 17; yspectra_every = 3;")
    assert d.yspectra_every == 3 and d.yspectra_pressure == 0
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, yspectra_every=-1)
    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, yspectra_pressure=2)
