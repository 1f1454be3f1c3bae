"""Opt-in kernel variants behind environment switches, each checked in a fresh child process (the
switches are read once per process): CHANNEL_ZFFT (z-stage row plans, incl. the paired-row H_z of
ZFFT=4 on odd row counts) against NumPy, CHANNEL_KSPEC_W8 (K-SPEC at 8 lines, two waves per SIMD)
against the fp64 oracle, the K-SPEC A/B variants CHANNEL_KSPEC_SPLIT (advance + output kernel, combine
mode), CHANNEL_KSPEC_GLDS7, CHANNEL_KSPEC_NS7 (R = 7 fp32) and CHANNEL_KSPEC_VAR = w4 | ns2 | ns5 | ns7
(R = 3) against the oracle in state and plane statistics, each asserting the kernel it launched
(kspec_last_variant), CHANNEL_XSEGROWS=0 (per-element exchange-segment lookups of the P > 1 x
kernels) bitwise against the single-rank fast path.  README "Environment switches" lists them."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZSTAGE_SCRIPT = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
from channel_gpu_amd import require_native
C = require_native()
rng = np.random.default_rng(7)
Nzp = 1024
nkz = Nzp // 3 + 1
for dtype, tol in ((torch.complex64, 5e-6), (torch.complex128, 1e-12)):
    # rows = ny * NX (a multiple of the block's 4 rows): 48 and 40 rows give every wave of the
    # persistent grid one row (ZFFT=4: the unpaired tail path), 3072 rows more groups than the
    # grid holds (blocks walk one or two groups: paired and unpaired waves)
    for NX, ny in ((16, 3), (8, 5), (64, 48)):
        f = rng.standard_normal((6, ny, NX, nkz)) + 1j * rng.standard_normal((6, ny, NX, nkz))
        f[..., 0] = f[..., 0].real
        H, m = C.zphys(torch.tensor(f, dtype=dtype, device="cuda"), Nzp, torch.ones(ny, dtype=torch.float64), 1.0, 1.0)
        phys = np.fft.irfft(np.concatenate([f, np.zeros(f.shape[:-1] + (Nzp // 2 + 1 - nkz,))], -1), n=Nzp,
                            axis=-1, norm="forward")
        u, v, w, wx, wy, wz = phys
        Hp = np.stack([v * wz - w * wy, w * wx - u * wz, u * wy - v * wx])
        Href = np.fft.rfft(Hp, axis=-1, norm="forward")[..., :nkz] / NX
        e = np.linalg.norm(H.cpu().numpy() - Href) / np.linalg.norm(Href)
        assert e < tol, (dtype, NX, ny, e)
        assert abs(m.cpu().numpy()[0] - np.abs(u).max()) < 1e-4 * np.abs(u).max()
print("ZSTAGE_OK")
"""


def _child(script, env_extra, token, timeout=300):
    env = dict(os.environ, CHANNEL_ROOT=ROOT, **env_extra)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and token in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("mode", ["0", "1", "2", "4"])
def test_zfft_row_plans(mode):
    """CHANNEL_ZFFT = 0 (LDS twiddles), 1 (register twiddles), 2 (16 x 16 x 4 with pad-per-32 rows),
    4 (paired-row H_z: two rows' H_z as one transform, the odd row of a wave through hzbuf, alone);
    the default 3 runs in test_kernels_gpu.py::test_zphys."""
    _child(ZSTAGE_SCRIPT, {"CHANNEL_ZFFT": mode}, "ZSTAGE_OK")


W8_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
from channel_gpu_amd import require_native
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config
C = require_native()
NX, NY, NZ, dt = 16, 385, 9, 1e-4
cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision="fp32", dt_fixed=dt, stats_every=0, log_every=0,
                     symmetry_every=0, ic="zero")
s = C.Solver(cfg, 0, 1, 0, b"")
o = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=dt)
phi, om = ora.random_state(o.plan, o.ops, seed=5, amp=0.05)
phi = phi.astype(np.complex64).astype(np.complex128)
om = om.astype(np.complex64).astype(np.complex128)
U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
o.set_state(phi, om, U)
s.set_state(phi, om, U)
s.prepare()
rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
for it in range(2):
    o.step()
    s.step(False)
    gphi, gom, gU = s.get_state()
    assert rel(gphi, o.phi) < 1e-4 and rel(gom, o.om) < 1e-4 and rel(gU, o.U) < 1e-5, (it, rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U))
print("W8_OK")
"""


def test_kspec_w8_matches_oracle():
    """CHANNEL_KSPEC_W8=1: the R = 7 fp32 K-SPEC at 8 lines per workgroup (LEAN 2-RHS solves, async
    LDS staging) against the fp64 oracle at the one-wave kernel's fp32 tolerance
    (test_solver_gpu.py::test_gpu_matches_oracle_large_ny[fp32-385])."""
    _child(W8_SCRIPT, {"CHANNEL_KSPEC_W8": "1"}, "W8_OK")


KSPEC_SWITCH_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHANNEL_ROOT"], "tests"))
import refchecks as rc
from channel_gpu_amd import require_native
from channel_gpu_amd.reference import oracle as ora
from channel_gpu_amd.utils.config import default_config
C = require_native()
NY, precision, variant = int(os.environ["SW_NY"]), os.environ["SW_PRECISION"], os.environ["SW_VARIANT"]
NX, NZ, dt = 16, 9, 1e-4
cfg = default_config(NX=NX, NY=NY, NZ=NZ, Re=400.0, precision=precision, dt_fixed=dt, stats_every=1, log_every=0,
                     symmetry_every=0, ic="zero")
s = C.Solver(cfg, 0, 1, 0, b"")
o = ora.OracleSolver(NX, NY, NZ, Re=400.0, dt_fixed=dt)
phi, om = ora.random_state(o.plan, o.ops, seed=5, amp=0.05)
if precision == "fp32":
    phi = phi.astype(np.complex64).astype(np.complex128)
    om = om.astype(np.complex64).astype(np.complex128)
U = 0.75 * 1.8 * (1 - o.ops.y ** 2)
o.set_state(phi, om, U)
s.set_state(phi, om, U)
s.prepare()
o.prepare()
assert C.kspec_last_variant() == variant, C.kspec_last_variant()
rc.assert_stats_sensitive(o)
stol = rc.stats_tol(precision, NY)
tol, tolU = (1e-9, 1e-11) if precision == "fp64" else (1e-4 * max(1.0, NY / 600), 1e-5)
e = rc.stats_errors(s.stats(), o.plane_stats())
print("STATS_ERR", precision, NY, variant, "prepare", e)
assert max(e) < stol, ("prepare()", e)
rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
for it in range(2):
    o.step()
    s.step(True)
    assert C.kspec_last_variant() == variant, C.kspec_last_variant()
    gphi, gom, gU = s.get_state()
    es = rel(gphi, o.phi), rel(gom, o.om), rel(gU, o.U)
    e = rc.stats_errors(s.stats(), o.plane_stats())
    print("STATS_ERR", precision, NY, variant, "step", it, e, "state", es)
    assert es[0] < tol and es[1] < tol and es[2] < tolU, (it, es)
    assert max(e) < stol, ("step(True)", it, e)
assert s.health() == 0
print("KSPEC_SWITCH_OK")
"""

SPLIT_NOTE = "CHANNEL_KSPEC_SPLIT ignored"


def _kspec_switch(env, NY, precision, variant, note=False):
    env = dict(os.environ, CHANNEL_ROOT=ROOT, SW_NY=str(NY), SW_PRECISION=precision, SW_VARIANT=variant, **env)
    r = subprocess.run([sys.executable, "-c", KSPEC_SWITCH_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "KSPEC_SWITCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert (SPLIT_NOTE in r.stderr) == note, r.stderr[-2000:]
    assert r.stderr.count(SPLIT_NOTE) <= 1  # (a one-time note)


@pytest.mark.parametrize("NY,R", [(289, 5), (385, 7)])
def test_kspec_split_matches_oracle(NY, R):
    """CHANNEL_KSPEC_SPLIT=1 in the combine mode (CHANNEL_COMBINE=1), fp32: the advance kernel stops
    after the phi / v stores and kspec_out_kernel forms D1 v, D1 omega and the statistics from the
    stored fields with its own row map.  Two steps against the oracle: state at the fp32 tolerance of
    test_gpu_matches_oracle_large_ny, prepare() and step(True) statistics at refchecks.stats_tol."""
    _kspec_switch({"CHANNEL_KSPEC_SPLIT": "1", "CHANNEL_COMBINE": "1"}, NY, "fp32",
                  f"kspec_kernel<{R}, float, 4, 2, 2, 0, 0, 1, 1> + kspec_out_kernel<{R}, float, 8, 2>")


def test_kspec_split_ignored_in_six_output_mode():
    """CHANNEL_KSPEC_SPLIT=1 without the combine mode (the one-rank default writes the six fields, which
    the output kernel does not): the fused kernel runs, and says so once on stderr, so that an A/B
    run cannot measure the wrong kernel silently."""
    _kspec_switch({"CHANNEL_KSPEC_SPLIT": "1"}, 385, "fp32", "kspec_kernel<7, float, 4, 2, 2, 0, 0, 0, 1>", note=True)


@pytest.mark.parametrize("env,variant", [
    ({"CHANNEL_KSPEC_GLDS7": "1"}, "kspec_kernel<7, float, 4, 2, 2, 0, 1, 0, 1>"),
    ({"CHANNEL_KSPEC_NS7": "3"}, "kspec_kernel<7, float, 4, 3, 2, 0, 0, 0, 1>"),
], ids=["glds7", "ns7=3"])
def test_kspec_r7_variants_match_oracle(env, variant):
    """The R = 7 fp32 A/B variants at NY = 385: async LDS staging in place of the two register slots
    (CHANNEL_KSPEC_GLDS7=1), three register prefetch slots (CHANNEL_KSPEC_NS7=3)."""
    _kspec_switch(env, 385, "fp32", variant)


@pytest.mark.parametrize("var,precision,W,NS", [("w4", "fp64", 4, 1), ("ns2", "fp64", 8, 2), ("ns5", "fp64", 8, 5),
                                                ("ns7", "fp64", 8, 7), ("w4", "fp32", 4, 1)])
def test_kspec_r3_variants_match_oracle(var, precision, W, NS):
    """CHANNEL_KSPEC_VAR at NY = 129 (R = 3): 4 lines per workgroup with one slot (w4), or 8 lines
    with 2 / 5 / 7 register prefetch slots."""
    T = "double" if precision == "fp64" else "float"
    _kspec_switch({"CHANNEL_KSPEC_VAR": var}, 129, precision, f"kspec_kernel<3, {T}, {W}, {NS}, 2, 0, 0, 0, 1>")


SEGROWS_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["CHANNEL_ROOT"])
from channel_gpu_amd import require_native
from channel_gpu_amd.utils.config import default_config
C = require_native()
res = []
for uid in (b"", C.new_unique_id()):
    cfg = default_config(NX=64, NY=65, NZ=33, Re=1000.0, precision="fp64", ic="random", ic_amplitude=0.2,
                         stats_every=0, log_every=0, symmetry_every=0)
    s = C.Solver(cfg, 0, 1, 0, uid)
    s.init_ic()
    s.prepare()
    for _ in range(3):
        s.step(False)
    res.append(s.get_state())
    del s
for a, b in zip(res[0], res[1]):
    assert np.array_equal(a, b)
print("SEGROWS_OK")
"""


@pytest.mark.parametrize("combine", ["0", "1"])
def test_xsegrows_off_is_bitwise(combine):
    """CHANNEL_XSEGROWS=0: the P > 1 x kernels (1-rank RCCL communicator, 4 kx sub-blocks = 4
    exchange segments incl. the self blocks) with per-element segment lookups instead of the
    per-thread row tables, bitwise against the single-rank fast path; with K-SPEC's six outputs
    and in the combine mode (CHANNEL_COMBINE=1 on both sides)."""
    _child(SEGROWS_SCRIPT, {"CHANNEL_XSEGROWS": "0", "CHANNEL_COMBINE": combine}, "SEGROWS_OK")
