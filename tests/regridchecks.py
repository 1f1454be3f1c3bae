"""Shared inputs of the regridding tests (test_regrid_cpu.py, test_regrid_gpu.py): source states on
small grids, restart files written from NumPy arrays with the bound HDF5 writers (no solver needed to
make an input), and the NumPy reference of the result."""
import functools
import os

import numpy as np

from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.reference import regrid as rg

SMALL = (32, 33, 17, 2.0)      # the source of most cases
XZ = (48, 33, 25, 2.0)         # x/z only: the same y grid
FINE = (48, 49, 25, 1.6)       # every direction and another stretch
GARBAGE = 1e30                 # what the source files hold in the dealiased band


def dims(grid):
    NX, NY, NZ = grid[:3]
    return NY, 2 * (NX // 3) + 1, (2 * NZ - 2) // 3 + 1


@functools.lru_cache(maxsize=None)
def source_state(grid=SMALL, seed=5, amp=0.3, Q=1.8):
    """(phi, om, U) of oracle.random_state on the grid, as a restart file of that grid decodes it: the
    file holds N2 * f in doubles and a reader divides by N2 again."""
    NX, NY, NZ, stretch = grid
    plan = ora.OraclePlan(NX, NY, NZ)
    ops = ora.build_ops(NY, stretch)
    phi, om = ora.random_state(plan, ops, seed=seed, amp=amp)
    U = 0.75 * Q * (1.0 - rg.tanh_grid(NY, stretch) ** 2)
    N2 = float(NX * (2 * NZ - 2))
    dec = lambda f: (f * N2) / N2  # noqa: E731
    out = dec(phi.real) + 1j * dec(phi.imag), dec(om.real) + 1j * dec(om.imag), dec(U)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(src=SMALL, dst=FINE, width=6, seed=5, amp=0.3):
    out = rg.regrid_state(*source_state(src, seed, amp), src=src, dst=dst, width=width)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def smooth_state(grid):
    """An analytic state for the large-NY layout cases (no dense y operators to build): every line a
    different smooth complex profile with non-zero values at the walls in phi, file-decoded like
    source_state.  Not Hermitian: for loading and reading back, not for stepping."""
    NX, NY, NZ, stretch = grid
    _, nkx, nkz = dims(grid)
    y = rg.tanh_grid(NY, stretch)[:, None, None]
    i = np.arange(nkx)[None, :, None]
    k = np.arange(nkz)[None, None, :]
    phi = (1.0 + 0.1 * i) * np.exp(1j * (3.0 * y + 0.3 * i + 0.7 * k)) / (1.0 + k) + 0.25 * y ** 3
    om = (1.0 - y ** 2) * np.exp(1j * (5.0 * y * y - 0.2 * i + 0.4 * k)) * (1.0 + 0.05 * k)
    om[:, 0, 0] = 0.0  # (the mean line of the omega field holds U)
    U = 0.75 * 1.8 * (1.0 - y[:, 0, 0] ** 2) + 0.01 * np.sin(4.0 * y[:, 0, 0])
    N2 = float(NX * (2 * NZ - 2))
    dec = lambda f: (f * N2) / N2  # noqa: E731
    out = dec(phi.real) + 1j * dec(phi.imag), dec(om.real) + 1j * dec(om.imag), dec(U)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def smooth_reference(src, dst):
    out = rg.regrid_state(*smooth_state(src), src=src, dst=dst)
    for a in out:
        a.setflags(write=False)
    return out


def write_files(C, d, state, grid, *, name="src", attrs=None, stretch_attr=True, umean_in_g=True, box=None, garbage=True):
    """G / DDV files of the state on the grid (float64 datasets), the retained modes in N2 units and
    `GARBAGE` everywhere else (the dealiased planes and kz columns a regrid must never read)."""
    phi, om, U = state
    NX, NY, NZ, stretch = grid
    NYd, nkx, nkz = dims(grid)
    Kx, N2 = NX // 3, float(NX * (2 * NZ - 2))
    g, ddv = os.path.join(str(d), name + "_G.h5"), os.path.join(str(d), name + "_DDV.h5")
    retained = [i if i <= Kx else NX - (nkx - i) for i in range(nkx)]
    a = dict(time=3.7, dt=0.004, step=12.0, Re=400.0, Q=1.8, NX=float(NX), NY=float(NY), NZ=float(NZ))
    a.update(box or dict(LX=2 * np.pi, LZ=np.pi))
    if stretch_attr:
        a["stretch"] = stretch
    if attrs is not None:
        a = attrs
    for path, f in ((g, om), (ddv, phi)):
        C.h5_create_field(path, NX, NY, NZ, True, -1)
        data = np.full((NX, NZ, NY, 2), GARBAGE if garbage else 0.0)
        data[retained, :nkz, :, 0] = np.transpose(f.real * N2, (1, 2, 0))
        data[retained, :nkz, :, 1] = np.transpose(f.imag * N2, (1, 2, 0))
        C.h5_write_planes(path, list(range(NX)), data.reshape(-1))
        if a:
            C.h5_write_attrs(path, a)
    if umean_in_g:
        C.h5_write_vector(g, "umean", np.asarray(U) * N2)
    return g, ddv


def config(grid, precision="fp64", **kw):
    from channel_gpu_amd.utils.config import default_config

    NX, NY, NZ, stretch = grid
    base = dict(NX=NX, NY=NY, NZ=NZ, stretch=stretch, Re=400.0, precision=precision, dt_fixed=0.01, ic="zero",
                stats_every=0, log_every=0, symmetry_every=0)
    base.update(kw)
    return default_config(**base)


def maxerr(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max())
