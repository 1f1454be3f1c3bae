"""The z stage's per-wave LDS slot (zphys_kernel DMA: pair 1 of a wave's next row copied global -> LDS
a row ahead) at Nzp = 1024, complex64, nkz = 342, on the smallest row counts that reach each state of
its pipeline:

  NX x ny   rows   grid             state
  16 x 3      48   default          one row per wave: prologue copy and the last row's dummy copy only
   8 x 5      40   default          fewer row groups than blocks
  64 x 24   1536   CHANNEL_Z_BPC=1  384 groups over 256 blocks: blocks with two rows beside blocks with one
  64 x 48   3072   CHANNEL_Z_BPC=1  three rows per wave (the headline's count per launch): the slot is reused twice

The slot is opt-in (CHANNEL_ZDMA=1: it did not beat the register-only prefetch on the headline grid,
profiles/zdma/README.md).  Four child processes (CHANNEL_ZDMA, CHANNEL_ZFFT and CHANNEL_LDS_POISON are
read once per process; CHANNEL_Z_BPC is read per launch and set inside the child) run every shape once
on the same input and leave H, the maxima and zphys_last_variant() in a file; the tests compare those:
the slot against NumPy (as test_kernels_gpu.py::test_zphys) and bitwise against the default (the
register-only prefetch: the data path changes, not the arithmetic) and against the LDS poison fill;
the slot under the paired-row plan CHANNEL_ZFFT=4 against NumPy.  One call with an odd nkz takes the
segment kernel and says so."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NZP = 1024
NKZ = NZP // 3 + 1
SHAPES = [(16, 3, ""), (8, 5, ""), (64, 24, "1"), (64, 48, "1")]  # (NX, ny, CHANNEL_Z_BPC)
SLOT = "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, true>"
SLOT4 = "zphys_kernel<1024, float, false, true, 64, 4, 2, 4, true>"
REGS = "zphys_kernel<1024, float, false, true, 64, 4, 2, 3, false>"

CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHANNEL_ROOT"], "tests"))
from channel_gpu_amd import require_native
from test_zphys_dma_gpu import SHAPES, NZP, fields
C = require_native()
out = {}
for NX, ny, bpc in SHAPES:
    if bpc:
        os.environ["CHANNEL_Z_BPC"] = bpc
    else:
        os.environ.pop("CHANNEL_Z_BPC", None)
    f = fields(NX, ny)
    H, m = C.zphys(torch.tensor(f, dtype=torch.complex64, device="cuda"), NZP, torch.ones(ny, dtype=torch.float64), 1.0, 1.0)
    out[f"H_{NX}_{ny}"] = H.cpu().numpy()
    out[f"m_{NX}_{ny}"] = m.cpu().numpy()
    out[f"v_{NX}_{ny}"] = np.array(C.zphys_last_variant())
os.environ.pop("CHANNEL_Z_BPC", None)
# an odd nkz (not Nzp / 3 + 1): the segment kernel, whatever CHANNEL_ZDMA says
f = fields(16, 3, NZP // 3)
H, m = C.zphys(torch.tensor(f, dtype=torch.complex64, device="cuda"), NZP, torch.ones(3, dtype=torch.float64), 1.0, 1.0)
out["H_odd"] = H.cpu().numpy()
out["v_odd"] = np.array(C.zphys_last_variant())
np.savez(os.environ["ZDMA_OUT"], **out)
print("ZDMA_CHILD_OK")
"""


def fields(NX, ny, nkz=NKZ):
    """The six input fields of a shape (the same in every child)."""
    rng = np.random.default_rng(1000 * NX + ny)
    f = rng.standard_normal((6, ny, NX, nkz)) + 1j * rng.standard_normal((6, ny, NX, nkz))
    f[..., 0] = f[..., 0].real  # kz = 0 coefficient of a real z-row
    return f


def reference(f):
    """H and the physical u, v, w of test_kernels_gpu.py::test_zphys."""
    nkz, NX = f.shape[-1], f.shape[2]
    phys = np.fft.irfft(np.concatenate([f, np.zeros(f.shape[:-1] + (NZP // 2 + 1 - nkz,))], -1), n=NZP, axis=-1,
                        norm="forward")
    u, v, w, wx, wy, wz = phys
    Hp = np.stack([v * wz - w * wy, w * wx - u * wz, u * wy - v * wx])
    return np.fft.rfft(Hp, axis=-1, norm="forward")[..., :nkz] / NX, (u, v, w)


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("zdma")
    res = {}
    for name, extra in (("slot", {"CHANNEL_ZDMA": "1"}), ("regs", {}),
                        ("poison", {"CHANNEL_ZDMA": "1", "CHANNEL_LDS_POISON": "1"}),
                        ("slot4", {"CHANNEL_ZDMA": "1", "CHANNEL_ZFFT": "4"})):
        path = str(d / (name + ".npz"))
        env = dict(os.environ, CHANNEL_ROOT=ROOT, ZDMA_OUT=path, **extra)
        for k in ("CHANNEL_ZDMA", "CHANNEL_LDS_POISON", "CHANNEL_Z_BPC", "CHANNEL_ZFFT"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ZDMA_CHILD_OK" in r.stdout, (name, r.stdout[-2000:], r.stderr[-3000:])
        res[name] = dict(np.load(path))
    return res


@pytest.mark.parametrize("NX,ny", [(s[0], s[1]) for s in SHAPES])
def test_slot_matches_numpy(runs, NX, ny):
    """CHANNEL_ZDMA=1: the slot variant ran (of the default row plan, and of the paired-row plan), H
    within the 5e-6 relative L2 of test_zphys, the four maxima within its 1e-4."""
    check_numpy(runs["slot"], SLOT, NX, ny)
    check_numpy(runs["slot4"], SLOT4, NX, ny)


def check_numpy(d, variant, NX, ny):
    assert str(d[f"v_{NX}_{ny}"]) == variant, d[f"v_{NX}_{ny}"]
    Href, (u, v, w) = reference(fields(NX, ny))
    e = rel(d[f"H_{NX}_{ny}"], Href)
    print(f"rel L2 {NX}x{ny}: {e:.3e}")
    assert e < 5e-6
    m = d[f"m_{NX}_{ny}"]
    for got, want in ((m[0], np.abs(u).max()), (m[1], np.abs(v).max()), (m[2], np.abs(w).max()),
                      (m[3], (np.abs(u) + np.abs(v) + np.abs(w)).max())):
        assert abs(got - want) < 1e-4 * want, (m, want)


@pytest.mark.parametrize("NX,ny", [(s[0], s[1]) for s in SHAPES])
def test_slot_bitwise_equals_register_prefetch(runs, NX, ny):
    """The default (register-only prefetch) on the same input: H and the maxima bitwise equal."""
    d, r = runs["slot"], runs["regs"]
    assert str(r[f"v_{NX}_{ny}"]) == REGS, r[f"v_{NX}_{ny}"]
    assert np.array_equal(d[f"H_{NX}_{ny}"].view(np.uint32), r[f"H_{NX}_{ny}"].view(np.uint32))
    assert np.array_equal(d[f"m_{NX}_{ny}"].view(np.uint32), r[f"m_{NX}_{ny}"].view(np.uint32))


@pytest.mark.parametrize("NX,ny", [(s[0], s[1]) for s in SHAPES])
def test_slot_bitwise_under_lds_poison(runs, NX, ny):
    """CHANNEL_LDS_POISON=1 fills the LDS (the slots included) with NaN first: the same bits come out,
    so no lane reads a slot byte that no copy wrote."""
    d, q = runs["slot"], runs["poison"]
    assert str(q[f"v_{NX}_{ny}"]) == SLOT, q[f"v_{NX}_{ny}"]
    assert np.array_equal(d[f"H_{NX}_{ny}"].view(np.uint32), q[f"H_{NX}_{ny}"].view(np.uint32))
    assert np.array_equal(d[f"m_{NX}_{ny}"].view(np.uint32), q[f"m_{NX}_{ny}"].view(np.uint32))


def test_odd_nkz_takes_the_fallback(runs):
    """nkz = 341: rows are no whole 16-byte pieces (and not the one-segment count), so the launcher
    takes the segment kernel without the slot even with CHANNEL_ZDMA=1, and says so; H still matches
    NumPy."""
    d = runs["slot"]
    assert str(d["v_odd"]) == "zphys_kernel<1024, float, true, true, 64, 4, 2, 3, false>", d["v_odd"]
    Href, _ = reference(fields(16, 3, NZP // 3))
    assert rel(d["H_odd"], Href) < 5e-6
