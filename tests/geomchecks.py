"""Shared geometries, states, references and preconditions of the tests on a non-default box, grid
stretching and flow rate (test_geometry_cpu.py, test_geometry_gpu.py, test_multirank_gpu.py).
NumPy only: nothing here calls the native core (solver() is handed the module by its caller).

The default box has ax = 2 pi / LX = 1, the multiplicative identity, and az = 2: a kernel that drops
ax, squares it once too few or reads its argument struct's defaults passes every default-box test.
GEOM_A has ax = 0.75, az = 1.6: none of ax, az, ax^2, az^2, ax az, 1 / ax, 1 / az equals another or
1, 2 or 4.  GEOM_B is the common production box 4 pi x 2 pi (az = 1: the identity on the other axis).

A comparison on GEOM_A only means something if the reference itself depends on the geometry, so
every compared quantity first passes assert_geometry_sensitive: the NumPy reference, evaluated on
the same state arrays with one of MUTATIONS applied to the geometry, must move by >= SENSITIVITY."""
import functools
import math

import numpy as np

from channel_gpu_amd.reference import budgets as bud
from channel_gpu_amd.reference import cross_spectra as xsp
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import pressure as prs
from channel_gpu_amd.reference import spectra as spc
from channel_gpu_amd.reference import spectral_budgets as sbr
from channel_gpu_amd.utils.config import default_config

GEOM_A = dict(LX=8 * math.pi / 3, LZ=5 * math.pi / 4, stretch=1.6, Q=1.3)
GEOM_B = dict(LX=4 * math.pi, LZ=2 * math.pi)
DEFAULTS = dict(LX=2 * math.pi, LZ=math.pi, stretch=2.0, Q=1.8)

RE = 400.0
# 100 x the loosest fp32 state tolerance (1e-4), 1000 x the fp32 diagnostics tolerance (1e-5)
SENSITIVITY = 1e-2


def full(geom):
    """geom with the defaults of the keys it leaves out."""
    return {**DEFAULTS, **geom}


def _swap(g):
    return {**g, "LX": g["LZ"], "LZ": g["LX"]}


# what a device path that ignored, defaulted or swapped a key would compute
MUTATIONS = {
    "LX -> 2 pi": lambda g: {**g, "LX": 2 * math.pi},
    "LZ -> pi": lambda g: {**g, "LZ": math.pi},
    "LX <-> LZ": _swap,
    "stretch -> 2.0": lambda g: {**g, "stretch": 2.0},
    "Q -> 1.8": lambda g: {**g, "Q": 1.8},
}
BOX = ("LX -> 2 pi", "LZ -> pi", "LX <-> LZ")          # every quantity with a wavenumber in it
BOX_Y = BOX + ("stretch -> 2.0",)                       # ... that also passes through a y operator
ALL = BOX_Y + ("Q -> 1.8",)                             # the step's U


def mutated(geom, name):
    """The full geometry after mutation `name`, or None where the mutation changes nothing (GEOM_B
    keeps the default stretch and Q)."""
    g = full(geom)
    m = MUTATIONS[name](g)
    return None if m == g else m


def change(got, ref):
    """The largest row-wise max-normalised change: max over the rows (first axis; a vector is one row)
    of max |got - ref| / max |ref|; rows whose reference vanishes (wall planes) do not count."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    a = got.reshape(got.shape[0], -1) if got.ndim > 1 else got.reshape(1, -1)
    b = ref.reshape(a.shape)
    num, den = np.abs(a - b).max(axis=1), np.abs(b).max(axis=1)
    keep = den > 1e-12 * max(den.max(), 1e-300)
    return float((num[keep] / den[keep]).max())


def make_oracle(NX, NY, NZ, geom, **kw):
    return ora.OracleSolver(NX, NY, NZ, Re=RE, **full(geom), **kw)


def make_state(NX, NY, NZ, geom, seed, amp, fp32=False, smooth=False):
    """(phi, omega, U) of the suite's random state on the geometry's own wavenumbers and y grid, with
    the parabola of the geometry's flux; complex64-rounded for fp32 storage; read-only."""
    g = full(geom)
    plan = ora.OraclePlan(NX, NY, NZ, LX=g["LX"], LZ=g["LZ"])
    ops = ora.build_ops(NY, g["stretch"])
    phi, om = (bud.smooth_state if smooth else ora.random_state)(plan, ops, seed=seed, amp=amp)
    if fp32:
        phi = phi.astype(np.complex64).astype(np.complex128)
        om = om.astype(np.complex64).astype(np.complex128)
    U = 0.75 * g["Q"] * (1 - ops.y ** 2)
    for a in (phi, om, U):
        a.setflags(write=False)
    return phi, om, U


def make_config(NX, NY, NZ, geom, precision, **kw):
    return default_config(NX=NX, NY=NY, NZ=NZ, Re=RE, precision=precision, **geom,
                          **{"ic": "zero", "stats_every": 0, "log_every": 0, "symmetry_every": 0, **kw})


def make_solver(native, NX, NY, NZ, geom, precision, uid=b"", **kw):
    """The native solver on `geom`; the caller sets the state (make_state) and calls prepare()."""
    cfg = make_config(NX, NY, NZ, geom, precision, **kw)
    g = full(geom)
    assert (cfg.LX, cfg.LZ, cfg.stretch, cfg.Q) == (g["LX"], g["LZ"], g["stretch"], g["Q"])
    return native.Solver(cfg, 0, 1, 0, uid)


def assert_geometry_sensitive(compute, geom, state, which, grid, floor=SENSITIVITY, **kw):
    """Precondition on the reference alone.  compute(oracle) -> dict of arrays is evaluated on the
    oracle of `geom` and of every mutation in `which`, all given the same state arrays; every
    mutation must move every returned array by >= floor (change()).  `which` may be a tuple of
    mutation names for all arrays or a dict {array name: tuple}.  Returns the measured changes
    {mutation: {array: change}}."""
    NX, NY, NZ = grid

    def run(g):
        o = ora.OracleSolver(NX, NY, NZ, Re=RE, **g, **kw)
        o.set_state(*state)
        return compute(o)

    ref = run(full(geom))
    names = set(which) if not isinstance(which, dict) else set().union(*which.values())
    out = {}
    for name in MUTATIONS:
        if name not in names:
            continue
        g = mutated(geom, name)
        if g is None:
            continue
        got = run(g)
        out[name] = {}
        for k in ref:
            wanted = which.get(k, ()) if isinstance(which, dict) else which
            if name not in wanted:
                continue
            d = change(got[k], ref[k])
            out[name][k] = d
            assert d >= floor, f"the reference cannot tell '{name}' from {geom}: moves {k} by {d:.2e}"
    return out


# ---- whole steps ----------------------------------------------------------------------------------
# (NX, NY, NZ, geometry, precision, dt, seed, amp): the single-process step cases of
# test_geometry_gpu.py; test_geometry_cpu.py holds the preconditions on exactly these.
NSTEPS = 3
SMALL = (32, 33, 17)
R7 = (16, 385, 9)     # the smallest shapes that reach the R = 7 blocked layout and the R = 10 kernel
R10 = (16, 633, 9)
# grid: (dt, seed, amp).  The small grid as test_gpu_matches_oracle_fp64.  The tall lines take the
# step and seed of test_gpu_matches_oracle_large_ny (the random state is noise in y, and its CFL limit
# at these NY is 8e-4) and twice its amplitude: at amp = 0.05 the Reynolds stress moves U by only
# 6e-3 under 'LZ -> pi' in three steps of 1e-4 (NY = 385), below the floor; it grows with amp^2.
STEP_STATES = {SMALL: (0.01, 3, 0.3), R7: (1e-4, 5, 0.1), R10: (1e-4, 5, 0.1)}
# the distinct (grid, geometry, fp32 state) of the step cases, each under its own id
STEP_REFERENCES = {
    "small-A-fp64": (SMALL, GEOM_A, False),
    "small-A-fp32": (SMALL, GEOM_A, True),
    "small-B-fp64": (SMALL, GEOM_B, False),
    "r7-A-fp32": (R7, GEOM_A, True),
    "r10-A-fp64": (R10, GEOM_A, False),
}


def step_state(grid, geom, fp32):
    dt, seed, amp = STEP_STATES[grid]
    return dt, make_state(*grid, geom, seed, amp, fp32=fp32)


def steps(o, n=NSTEPS):
    """The state after n steps, and the plane statistics of the prepared and of the final state (the
    split K-SPEC case compares them: its output kernel's wavenumbers enter nothing else)."""
    o.prepare()
    st0 = o.plane_stats()
    for _ in range(n):
        o.step()
    return dict(phi=o.phi, omega=o.om, U=o.U, stats0=st0, stats=o.plane_stats())


STEP_WHICH = dict(phi=BOX_Y, omega=BOX_Y, U=ALL, stats0=BOX_Y, stats=BOX_Y)

# test_multirank_gpu.py: its grid, state (seed 5, amp 0.3), step and step count
MULTIRANK = dict(grid=SMALL, dt=0.01, seed=5, amp=0.3, nsteps=2)


# ---- diagnostics ------------------------------------------------------------------------------------
DIAG_SEED, DIAG_AMP = 9, 0.3          # the state of every diagnostics test file
CROSS_REFS = (3, 16)
SPECTRA_PLANES = (16, 4)
NAMES = ("u", "v", "w", "wx", "wy", "wz")


def numpy_spectra(o, planes):
    """ekx [3, np, Kx + 1], ekz [3, np, nkz] and the (kx, kz) map of the first plane, of u, v, w at
    `planes`, the mean line excluded (test_spectra_gpu.py)."""
    p = o.plan
    F = o.fields[:3]
    kx = np.asarray(p.kx_of(np.arange(p.nkx)))
    kz = np.arange(p.nkz)
    w = np.where(kz == 0, 1.0, 2.0)[None, :] * np.ones((p.nkx, 1))
    w[(kx == 0), 0] = 0.0
    ekx = np.zeros((3, len(planes), p.Kx + 1))
    ekz = np.zeros((3, len(planes), p.nkz))
    for i, j in enumerate(planes):
        e = np.abs(F[:, j]) ** 2 * w
        ekz[:, i] = e.sum(axis=1)
        for ig in range(p.nkx):
            ekx[:, i, abs(kx[ig])] += e[:, ig].sum(axis=-1)
    m = np.abs(F[:, planes[0]]) ** 2
    m[:, 0, 0] = 0.0
    return ekx, ekz, m


def numpy_moments(ph, U):
    """The eleven one-point moments of u' = u - U, v, w [3, NY, NX, Nzp] (test_physfields_gpu.py)."""
    u = ph[0] - U[:, None, None]
    v, w = ph[1], ph[2]
    rows = [u, u * u, v * v, w * w, u * v, u ** 3, v ** 3, w ** 3, u ** 4, v ** 4, w ** 4]
    return np.stack([r.mean(axis=(1, 2)) for r in rows])


def diagnostics(o):
    """Every reference of the diagnostics comparisons, of the oracle's prepared state."""
    o.prepare()
    d = dict(o=o)
    d["stats"] = np.asarray(o.plane_stats())
    d["spec_ekx"], d["spec_ekz"], d["spec_map"] = numpy_spectra(o, list(SPECTRA_PLANES))
    d["grad"] = bud.gradient_sums(o)
    ph = ora.spec_to_phys_full(o.fields, o.plan)
    d["phys"] = ph
    d["tri"] = bud.transport_moments(ph, o.U)
    d["moments"] = numpy_moments(ph[:3], o.U)
    Pi = prs.pressure_hat(o)
    d["Pi"] = Pi.reshape(o.phi.shape)
    d["pp"] = prs.pressure_physical(o, Pi)
    d["pmom"] = prs.pressure_moments(o, Pi)
    p_hat = prs.static_pressure_hat(o, Pi)
    d["p_hat"] = p_hat
    d["pstrain"] = prs.pressure_strain(o, p_hat)
    sp = spc.plane_spectra(o, p_hat)
    d["ysp_ekx"], d["ysp_ekz"] = sp["ekx"], sp["ekz"]
    for rows in ("velocity", "shear"):
        c = xsp.plane_cross_spectra(o, list(CROSS_REFS), rows)
        d[f"cross_{rows}"] = c
        d[f"cross_{rows}_ckx"], d[f"cross_{rows}_ckz"] = c["ckx"], c["ckz"]
    H = prs.rotational_hat(o)
    sb = sbr.spectral_budgets(o, H=H)
    d["H"] = H.reshape((3,) + o.phi.shape)
    d["sb_ekx"], d["sb_ekz"] = sb["ekx"], sb["ekz"]
    return d


# arrays of diagnostics() that must feel every box mutation and the stretch (all pass a y operator:
# v comes from the Helmholtz solve, u, w and the vorticities from D1)
DIAG_ARRAYS = ("stats", "spec_ekx", "spec_ekz", "spec_map", "grad", "tri", "moments", "Pi", "pp", "pmom", "p_hat",
               "pstrain", "ysp_ekx", "ysp_ekz", "cross_velocity_ckx", "cross_velocity_ckz", "cross_shear_ckx",
               "cross_shear_ckz", "H", "sb_ekx", "sb_ekz")
# the physical fields one by one; omega_y is the state's omega itself: no wavenumber and no y operator
# in it, so no mutation can move it (it is compared all the same: its transform is the others')
PHYS_SENSITIVE = ("u", "v", "w", "wx", "wz")


def diagnostics_arrays(o):
    d = diagnostics(o)
    out = {k: d[k] for k in DIAG_ARRAYS}
    for i, n in enumerate(NAMES):
        if n in PHYS_SENSITIVE:
            out[f"phys_{n}"] = d["phys"][i]
    # the wall shear of the histograms: omega_x, omega_z on the two wall planes (the wall dy)
    out["wall_wx"], out["wall_wz"] = d["phys"][3][[0, -1]], d["phys"][5][[0, -1]]
    return out


# ---- time-step control --------------------------------------------------------------------------------
ADAPTIVE = dict(cfl=0.5, dt_max=0.05)


def first_adaptive_step(o):
    """The CFL maxima of the prepared state and the corrected and parity time steps they give."""
    from refchecks import dt_reference

    o.prepare()
    o.step()
    p = o.plan
    m = o.maxima
    par = dt_reference(m, o.cfl, o.dt_max, 0.0, 1, p.NX, p.NZ, p.LX, p.LZ, o.Re, p.NY)
    return dict(cflsum=m[3:], dt=np.array([min(o.cfl / m[3], o.dt_max)]), dt_c_parity=np.array([par[0]]),
                dt_v_parity=np.array([par[1]]))


# (the plain maxima |u|, |v|, |w| are compared too; the sum and the steps carry the factors.  The
# parity formulas use a uniform dy = 2 / (NY - 1): the stretch reaches dt_c only through the fields,
# and dt_v, a formula of the box alone, not at all.)
ADAPTIVE_WHICH = dict(cflsum=BOX_Y, dt=BOX_Y, dt_c_parity=BOX_Y, dt_v_parity=BOX)


@functools.lru_cache(maxsize=None)
def diagnostics_reference(fp32=False):
    """State and references of the diagnostics cases (32 x 33 x 17 on GEOM_A), once per precision."""
    state = make_state(*SMALL, GEOM_A, DIAG_SEED, DIAG_AMP, fp32=fp32)
    o = make_oracle(*SMALL, GEOM_A)
    o.set_state(*state)
    d = diagnostics(o)
    d["state"] = state
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d
