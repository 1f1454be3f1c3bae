"""The one-rank layout of the x-expanded intermediates (rows of pitch xexp_pitch(nkz): whole 128-B
lines in fp32; CHANNEL_XEXP_LAYOUT=1) against rows of nkz (CHANNEL_XEXP_LAYOUT=0; the kernel entry points
called without a pitch).  Only addresses change, not arithmetic, and the CFL maxima are order-free, so every comparison
is bitwise:

  * the x-backward -> z -> x-forward chain through the tensor entry points (blocked spectral layout,
    K-SPEC's six outputs with the mean line of field 4 read as zero, non-temporal spectral accesses:
    what the solver launches on the headline grid), at the headline
    instantiation NX = Nzp = 1024, complex64, with ny = 3 (an odd plane count: the last plane tile of
    the x-forward is half empty), and at NX = Nzp = 32 (nkz = 11, a multiple of neither 8 nor 16; 8-byte
    accesses) in complex64 and complex128.  The padding columns kz >= nkz of the rows must come out as
    they went in (zeros): nobody stores to them;
  * two solver steps at 32x33x32 and 128x129x128: get_state(), the step log, one exported physical
    field and the pressure;
  * CHANNEL_ZDMA=1 (pair 1 of a wave's next row through the per-wave LDS slot) against the
    register-only prefetch under the padded pitch, in two child processes (CHANNEL_ZDMA is read once
    per process), each also against its own packed-row result; a third child does the same for the
    register-resident z stage (CHANNEL_ZREG=1), which takes the pitch as a kernel argument.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    """Bit pattern of a tensor or array, as unsigned bytes."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8)


def _chain(C, torch, N, ny, dtype, xpitch):
    """x-backward (six fields) -> z -> x-forward of ny planes at NX = Nzp = N; (phys, H, maxima, spec out)."""
    Kx, nkz = N // 3, N // 3 + 1
    nkx, nkzs, rows = 2 * Kx + 1, (nkz + 7) // 8 * 8, 8
    g = torch.Generator(device="cuda").manual_seed(1234 + N)
    rdt = torch.float32 if dtype == torch.complex64 else torch.float64
    spec = torch.view_as_complex(torch.randn(6 * rows * nkx * nkzs, 2, generator=g, device="cuda", dtype=rdt))
    phys = C.xfft_backward_blocked(spec, 6, rows, 0, ny, N, Kx, nkz, nt=1, zero_mean_field=4, xpitch=xpitch)
    assert phys.shape == (6, ny, N, xpitch or nkz)
    H, m = C.zphys(phys, N, torch.ones(ny, dtype=torch.float64), 1.0, 1.0, nkz=nkz if xpitch else 0)
    out = torch.zeros(3 * rows * nkx * nkzs, dtype=dtype, device="cuda")
    C.xfft_forward_blocked(H, out, rows, 0, Kx, nt=1, nkz=nkz if xpitch else 0)
    torch.cuda.synchronize()
    return phys, H, m, out, nkz


@pytest.mark.parametrize("N,ny,dtype", [(1024, 3, "complex64"), (32, 3, "complex64"), (32, 3, "complex128")])
def test_chain_bitwise_equals_packed_rows(native, N, ny, dtype):
    import torch

    dt = getattr(torch, dtype)
    pitch = native.xexp_pitch(N // 3 + 1)
    assert pitch % 16 == 0 and 0 <= pitch - (N // 3 + 1) < 16
    p0, H0, m0, s0, nkz = _chain(native, torch, N, ny, dt, 0)
    if N == 1024:  # the variants the headline grid runs
        assert native.xfft_last_backward_variant() == "xfft_backward_kernel<1024, float, false, 1, 0, 2, 2, false>"
        assert native.zphys_last_variant() in ("zphys_kernel<1024, float, false, true, 64, 4, 2, 3, false>",
                                               "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, true>")
    p1, H1, m1, s1, _ = _chain(native, torch, N, ny, dt, pitch)
    if N == 1024:
        assert native.xfft_last_backward_variant() == "xfft_backward_kernel<1024, float, false, 1, 0, 2, 2, false>"
        assert native.zphys_last_variant().endswith(", true>") and native.zphys_last_variant().count(",") == 9
    assert float(torch.abs(p0).max()) > 0 and float(torch.abs(s0).max()) > 0
    # the data columns of every stage, the maxima and the spectral result
    assert np.array_equal(_bits(p1[..., :nkz]), _bits(p0))
    assert np.array_equal(_bits(H1[..., :nkz]), _bits(H0))
    assert np.array_equal(_bits(m1), _bits(m0))
    assert np.array_equal(_bits(s1), _bits(s0))
    # the padding columns: still the zeros of the allocation after the x-backward and after the z stage
    assert pitch > nkz
    assert not _bits(p1[..., nkz:]).any()
    assert not _bits(H1[..., nkz:]).any()


def _two_steps(native, NX, NY, NZ, layout):
    from channel_gpu_amd.utils.config import default_config

    old = os.environ.get("CHANNEL_XEXP_LAYOUT")
    os.environ["CHANNEL_XEXP_LAYOUT"] = layout
    try:  # (the switch is read when a Solver allocates)
        cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=3250.0, precision="fp32", ic="random", ic_amplitude=0.2,
                             stats_every=0, log_every=0)
        s = native.Solver(cfg, 0, 1, 0, b"")
    finally:
        if old is None:
            os.environ.pop("CHANNEL_XEXP_LAYOUT", None)
        else:
            os.environ["CHANNEL_XEXP_LAYOUT"] = old
    s.init_ic()
    s.prepare()
    s.step(False)
    s.step(False)
    s.synchronize()
    L = s.log()
    log = {k: getattr(L, k) for k in dir(L) if not k.startswith("_") and isinstance(getattr(L, k), (int, float))}
    phi, om, U = s.get_state()
    f = s.physical_fields([0, NY // 2, NY - 2], ["wz", "p"])
    return phi, om, U, log, f["wz"].copy(), f["p"].copy()


@pytest.mark.parametrize("NX,NY,NZ", [(32, 33, 17), (128, 129, 65)])
def test_solver_steps_bitwise_equal(native, NX, NY, NZ):
    new = _two_steps(native, NX, NY, NZ, "1")
    old = _two_steps(native, NX, NY, NZ, "0")
    assert new[3] and new[3] == old[3], (new[3], old[3])
    assert new[3].get("health", 0) == 0
    for a, b, what in zip(new[:3] + new[4:], old[:3] + old[4:], ("phi", "omega", "U", "wz", "p")):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, what
        assert np.array_equal(_bits(a), _bits(b)), what


ZDMA_SHAPES = [(16, 3, ""), (64, 24, "1")]  # (NX, ny, CHANNEL_Z_BPC): one row per wave; blocks with two rows beside one
CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHANNEL_ROOT"], "tests"))
from channel_gpu_amd import require_native
from test_xexp_layout_gpu import ZDMA_SHAPES
C = require_native()
NZP, NKZ = 1024, 342
P = C.xexp_pitch(NKZ)
out = {}
for NX, ny, bpc in ZDMA_SHAPES:
    if bpc:
        os.environ["CHANNEL_Z_BPC"] = bpc
    else:
        os.environ.pop("CHANNEL_Z_BPC", None)
    rng = np.random.default_rng(77 * NX + ny)
    f = np.zeros((6, ny, NX, P), dtype=np.complex64)
    f[..., :NKZ] = rng.standard_normal((6, ny, NX, NKZ)) + 1j * rng.standard_normal((6, ny, NX, NKZ))
    f[..., 0] = f[..., 0].real
    idy = torch.ones(ny, dtype=torch.float64)
    H0, m0 = C.zphys(torch.tensor(f[..., :NKZ].copy(), device="cuda"), NZP, idy, 1.0, 1.0)
    out[f"v0_{NX}_{ny}"] = np.array(C.zphys_last_variant())
    H1, m1 = C.zphys(torch.tensor(f, device="cuda"), NZP, idy, 1.0, 1.0, nkz=NKZ)
    out[f"v1_{NX}_{ny}"] = np.array(C.zphys_last_variant())
    out[f"H0_{NX}_{ny}"] = H0.cpu().numpy()
    out[f"H1_{NX}_{ny}"] = H1.cpu().numpy()
    out[f"m0_{NX}_{ny}"] = m0.cpu().numpy()
    out[f"m1_{NX}_{ny}"] = m1.cpu().numpy()
np.savez(os.environ["XEXP_OUT"], **out)
print("XEXP_CHILD_OK")
"""


@pytest.fixture(scope="module")
def zdma_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("xexp")
    res = {}
    for name, extra in (("slot", {"CHANNEL_ZDMA": "1"}), ("regs", {}), ("zreg", {"CHANNEL_ZREG": "1"})):
        path = str(d / (name + ".npz"))
        env = dict(os.environ, CHANNEL_ROOT=ROOT, XEXP_OUT=path, **extra)
        for k in ("CHANNEL_ZDMA", "CHANNEL_ZREG", "CHANNEL_LDS_POISON", "CHANNEL_Z_BPC", "CHANNEL_ZFFT"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "XEXP_CHILD_OK" in r.stdout, (name, r.stdout[-2000:], r.stderr[-3000:])
        res[name] = dict(np.load(path))
    return res


@pytest.mark.parametrize("NX,ny", [(s[0], s[1]) for s in ZDMA_SHAPES])
def test_zdma_slot_under_padded_pitch(zdma_runs, NX, ny):
    slot, regs = zdma_runs["slot"], zdma_runs["regs"]
    k = f"_{NX}_{ny}"
    assert str(slot["v0" + k]) == "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, true>"
    assert str(slot["v1" + k]) == "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, true, true>"
    assert str(regs["v0" + k]) == "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, false>"
    assert str(regs["v1" + k]) == "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, false, true>"
    assert np.abs(regs["H0" + k]).max() > 0
    for d in (slot, regs):  # padded against packed rows, in the same process
        assert np.array_equal(_bits(d["H1" + k][..., :342]), _bits(d["H0" + k]))
        assert np.array_equal(_bits(d["m1" + k]), _bits(d["m0" + k]))
        assert not _bits(d["H1" + k][..., 342:]).any()
    # the slot against the register-only prefetch under the padded pitch
    assert np.array_equal(_bits(slot["H1" + k]), _bits(regs["H1" + k]))
    assert np.array_equal(_bits(slot["m1" + k]), _bits(regs["m1" + k]))


@pytest.mark.parametrize("NX,ny", [(s[0], s[1]) for s in ZDMA_SHAPES])
def test_register_stage_under_padded_pitch(zdma_runs, NX, ny):
    """CHANNEL_ZREG=1 (zphys_reg_kernel, its own arithmetic): padded against packed rows, bitwise."""
    d, k = zdma_runs["zreg"], f"_{NX}_{ny}"
    assert np.abs(d["H0" + k]).max() > 0
    assert np.array_equal(_bits(d["H1" + k][..., :342]), _bits(d["H0" + k]))
    assert np.array_equal(_bits(d["m1" + k]), _bits(d["m0" + k]))
    assert not _bits(d["H1" + k][..., 342:]).any()
    assert not np.array_equal(_bits(d["H0" + k]), _bits(zdma_runs["regs"]["H0" + k]))  # (really another kernel)
