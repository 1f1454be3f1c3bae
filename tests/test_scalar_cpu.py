"""The NumPy reference of the passive scalar (reference/scalar.py) against exact states, its own
invariants and the linear advection-diffusion rate of one mode; the configuration keys of the scalar.

32 x 33 x 17, Re = 400, Pr = 0.71 throughout."""
import functools

import numpy as np
import pytest

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import scalar as sca

G = dict(NX=32, NY=33, NZ=17, Re=400.0)


def _laminar(o):
    o.set_state(np.zeros_like(o.phi), np.zeros_like(o.om), 0.75 * o.Q * (1 - o.ops.y ** 2))


def test_conduction_profile_is_steady():
    o = sca.ScalarOracle(**G, dt_fixed=0.01, Pr=0.71, wall=(-1.0, 1.0))
    _laminar(o)
    o.set_scalar(o.laminar_scalar())
    assert np.abs(o.th[:, 0, 0].real - o.ops.y).max() < 1e-15
    for _ in range(5):
        o.step()
    drift = np.abs(o.th[:, 0, 0] - o.ops.y).max()
    rest = o.th.copy()
    rest[:, 0, 0] = 0
    print(f"conduction drift {drift:.2e}, other modes {np.abs(rest).max():.2e}")
    assert drift < 1e-12 and np.abs(rest).max() == 0.0


def test_internal_heating_profile_is_steady():
    o = sca.ScalarOracle(**G, dt_fixed=0.01, Pr=0.71, source=0.3)
    _laminar(o)
    want = 0.3 * (1 - o.ops.y ** 2) / (2 * o.kappa)
    o.set_scalar(o.laminar_scalar())
    assert np.allclose(o.th[:, 0, 0].real, want, rtol=0, atol=1e-13 * want.max())
    for _ in range(5):
        o.step()
    drift = np.abs(o.th[:, 0, 0].real - want).max() / want.max()
    print(f"heating relative drift {drift:.2e}")
    assert drift < 1e-12


@functools.lru_cache(maxsize=None)
def _random_run(Pr=0.71, flux=True, steps=3):
    o = sca.ScalarOracle(**G, dt_fixed=0.01, Pr=Pr, wall=(-1.0, 1.0))
    phi, om = ora.random_state(o.plan, o.ops, seed=3, amp=0.3)
    o.set_state(phi, om, 0.75 * 1.8 * (1 - o.ops.y ** 2))
    th0 = sca.random_scalar(o.plan, o.ops, seed=4, amp=0.2, mean=o.ops.y)
    o.set_scalar(th0)
    o.flux_on = flux
    out = [th0]
    for _ in range(steps):
        o.step()
        out.append(o.th.copy())
    for a in out:
        a.setflags(write=False)
    return o, out


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_random_state_invariants():
    o, th = _random_run()
    p = o.plan
    for k in range(1, 4):
        t = th[k]
        moved = _rel(t, th[k - 1])
        # kz = 0 plane: theta(-kx, 0) = conj theta(kx, 0)
        i = np.arange(1, p.Kx + 1)
        herm = np.abs(t[:, p.nkx - i, 0] - np.conj(t[:, i, 0])).max()
        print(f"step {k}: theta moves by {moved:.3e}, Hermitian defect {herm:.1e}")
        assert moved > 1e-3
        assert herm < 1e-14
        # wall rows exact: the Dirichlet values on the mean line, zero elsewhere
        assert t[0, 0, 0] == -1.0 and t[-1, 0, 0] == 1.0
        w = t[[0, -1]].copy()
        w[:, 0, 0] = 0
        assert np.array_equal(w, np.zeros_like(w))
        assert np.array_equal(t[:, 0, 0].imag, np.zeros(p.NY))


def test_passive_and_sensitive():
    """The momentum state is that of the plain oracle bitwise; theta sees Pr and the flux term at a
    level far above the 1e-9 of the device comparisons (their precondition)."""
    o, th = _random_run()
    b = ora.OracleSolver(**G, dt_fixed=0.01)
    phi, om = ora.random_state(b.plan, b.ops, seed=3, amp=0.3)
    b.set_state(phi, om, 0.75 * 1.8 * (1 - b.ops.y ** 2))
    for _ in range(3):
        b.step()
    assert np.array_equal(o.phi, b.phi) and np.array_equal(o.om, b.om) and np.array_equal(o.U, b.U)
    _, th_pr = _random_run(Pr=1.0)
    _, th_nf = _random_run(flux=False)
    s_pr, s_nf = _rel(th_pr[3], th[3]), _rel(th_nf[3], th[3])
    print(f"Pr = 1 instead of 0.71 moves theta by {s_pr:.3e}; dropping the flux term by {s_nf:.3e}")
    assert s_pr >= 1e-3
    assert s_nf >= 1e-3


def test_scalar_sums_are_plane_means():
    """Parseval: the sums equal the plane means of the physical-space products of the fluctuations."""
    o, th = _random_run()
    m = sca.scalar_sums(o)
    assert m.shape == (5, 33)
    f = o.fields[:3].copy()
    f[:, :, 0, 0] = 0
    t = o.th.copy()
    t[:, 0, 0] = 0
    uvw = ora.spec_to_phys_full(f, o.plan)
    tp = ora.spec_to_phys_full(t, o.plan)
    assert np.array_equal(m[0], o.th[:, 0, 0].real)
    want = np.stack([(tp * tp).mean(axis=(1, 2))] + [(uvw[c] * tp).mean(axis=(1, 2)) for c in range(3)])
    assert np.abs(m[1:] - want).max() < 1e-13 * np.abs(want).max()


def measured_rate(step, get, v, dt, nsteps):
    """Complex growth rate of the projection of theta's mode (1, 1) on the eigenvector over nsteps steps."""
    a0 = np.vdot(v, get())
    for _ in range(nsteps):
        step()
    a1 = np.vdot(v, get())
    return np.log(a1 / a0) / (nsteps * dt)


def test_linear_rate_matches_eigenvalue():
    dt, n = 0.002, 50
    lam, v = sca.linear_rate(NY=33, Re=400.0, Pr=0.71)
    o = sca.ScalarOracle(**G, dt_fixed=dt, Pr=0.71)
    _laminar(o)
    th = np.zeros_like(o.th)
    th[:, 1, 1] = 1e-3 * v
    o.set_scalar(th)
    rate = measured_rate(o.step, lambda: o.th[:, 1, 1], v, dt, n)
    print(f"measured rate {rate:.11f} against the eigenvalue {lam:.11f}: deviation {abs(rate - lam):.2e}")
    assert abs(rate - lam) < 1e-8
    # no other mode is excited
    rest = o.th.copy()
    rest[:, 1, 1] = 0
    assert np.abs(rest).max() < 1e-18


# ---- configuration ------------------------------------------------------------------------------------
def test_config_keys(native):
    from channel_gpu_amd.utils.config import config_from_string, default_config

    c = native.Config()
    assert (c.scalar, c.Pr, c.scalar_lower, c.scalar_upper, c.scalar_source, c.scalar_ic, c.in_T, c.out_T,
            c.scalar_every) == (False, 0.71, 0.0, 0.0, 0.0, "laminar", "-", "-", 0)
    c = default_config(NX=32, NY=33, NZ=17, scalar=True, Pr=2.5, scalar_lower=-1.0, scalar_upper=0.5, scalar_source=0.25,
                       scalar_ic="zero", out_T="t.h5", scalar_every=3)
    s = c.to_string()
    for line in ("scalar = true;", "Pr = 2.5;", "scalar_lower = -1;", "scalar_upper = 0.5;", "scalar_source = 0.25;",
                 'scalar_ic = "zero";', 'T = "t.h5";', "scalar_every = 3;"):
        assert line in s, line
    c2 = config_from_string(s)
    assert (c2.scalar, c2.Pr, c2.scalar_lower, c2.scalar_upper, c2.scalar_source, c2.scalar_ic, c2.in_T, c2.out_T,
            c2.scalar_every) == (True, 2.5, -1.0, 0.5, 0.25, "zero", "-", "t.h5", 3)
    # input.T implies scalar_ic = "file"
    c3 = config_from_string('NX = 32; NY = 33; NZ = 17; scalar = true; input: { T = "in.h5"; };')
    assert c3.in_T == "in.h5" and c3.scalar_ic == "file"
    # the defaults round-trip
    c4 = config_from_string(native.Config().to_string())
    assert not c4.scalar and c4.Pr == 0.71 and c4.scalar_ic == "laminar"


@pytest.mark.parametrize("bad", [dict(scalar=True, Pr=0.0), dict(scalar=True, Pr=-1.0),
                                 dict(scalar=True, regrid=True, in_T="t.h5"), dict(scalar=True, scalar_ic="random"),
                                 dict(scalar=True, scalar_every=-1), dict(scalar_every=2), dict(out_T="t.h5")])
def test_config_refusals(native, bad):
    from channel_gpu_amd.utils.config import default_config

    with pytest.raises(RuntimeError):
        default_config(NX=32, NY=33, NZ=17, **bad)
