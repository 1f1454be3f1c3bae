"""Cost of one plane_moments(), one plane_histograms() without and with the vorticity, one gradient_sums(), one transport_moments(), one pressure solve (the
device part of pressure_hat()), one pressure_moments(), one pressure_strain(), one plane_spectra() without and with
the pressure row, one spectral_budgets() and one three-field all-plane physical_fields() at 1024x385x1024 fp32, relative to one RK3 step in the same process.
--skip-fields leaves the (2 s, 10 GB of host memory) all-plane field export out; --pdfs-only stops after the
histograms; --sbudget-only runs the step, plane_spectra() and spectral_budgets() only; --ycross-only runs the
step, plane_spectra() and plane_cross_spectra() for 1, 4 and 16 reference planes only."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from channel_gpu_amd import require_core
from channel_gpu_amd.utils.config import default_config

C = require_core()
cfg = default_config(NX=1024, NY=385, NZ=513, Re=20700.0, precision="fp32", ic="random", ic_amplitude=0.05,
                     stats_every=0, log_every=0, symmetry_every=0)
s = C.Solver(cfg, 0, 1, 0, b"")
s.init_ic()
s.prepare()
for _ in range(5):
    s.step(False)
s.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    s.step(False)
s.synchronize()
step_ms = (time.perf_counter() - t0) * 100.0
res = {"grid": "1024x385x1024", "precision": "fp32", "step_ms": step_ms}

def spectral_budget_cost():
    """plane_spectra() and spectral_budgets(): host time of the whole calls, and the device time of the
    launches of the two stages by events, against the bytes they read (stage 0: the six fields, or five in
    the combine mode, and H_x, H_y, H_z; stage 1: u, v, w, omega_z, or the five, and Pi, p-hat')."""
    nkx, nkz = 2 * (cfg.NX // 3) + 1, (2 * cfg.NZ - 2) // 3 + 1
    nkzs = (nkz + 7) // 8 * 8 if s.spec_kzb() else nkz
    field = cfg.NY * nkx * nkzs * 8
    nf = 5 if s.combine() else 6
    res["plane_spectra_bytes"] = nf * field
    res["sbudget_stage0_bytes"] = (nf + 3) * field
    res["sbudget_stage1_bytes"] = ((5 if s.combine() else 4) + 2) * field
    res["sbudget_result_bytes"] = 20 * cfg.NY * (cfg.NX // 3 + 1 + nkz) * 8
    for name, call in (("plane_spectra", s.plane_spectra), ("spectral_budgets", s.spectral_budgets)):
        if name + "_ms" in res:  # (the full run has timed it above)
            continue
        ts = []
        for rep in range(5):
            t0 = time.perf_counter()
            r = call()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = ts
        res[name + "_over_step"] = min(ts) / step_ms
    tt = [s.spectral_budgets_timing() for _ in range(5)]
    for st in (0, 1):
        ms = [t[st] for t in tt]
        res[f"sbudget_stage{st}_ms"] = ms
        res[f"sbudget_stage{st}_TBps"] = res[f"sbudget_stage{st}_bytes"] / (min(ms) * 1e-3) / 1e12
    g, ps = s.gradient_sums(), s.pressure_strain()
    res["sbudget_g_uu_sum_vs_gradient_sums"] = float(abs(r["ekx"][4].sum(axis=-1) - g[3]).max() / abs(g[3]).max())
    res["sbudget_ps_uu_sum_vs_pstrain"] = float(abs(r["ekz"][14].sum(axis=-1) - ps[0]).max() / abs(ps[0]).max())


def cross_spectra_cost():
    """plane_cross_spectra() for 1, 4 and 16 reference planes of either row set: host time of the whole
    call, and the device time of its launches by events next to that of plane_spectra()'s in the same
    process, against the bytes they read (velocity: u, v, w, or the five fields of the combine mode; shear:
    also omega_z; the reference planes stay in cache)."""
    nkx, nkz = 2 * (cfg.NX // 3) + 1, (2 * cfg.NZ - 2) // 3 + 1
    nkzs = (nkz + 7) // 8 * 8 if s.spec_kzb() else nkz
    field = cfg.NY * nkx * nkzs * 8
    res["plane_spectra_bytes"] = (5 if s.combine() else 6) * field
    res["ycross_result_bytes_per_plane"] = 8 * cfg.NY * (cfg.NX // 3 + 1 + nkz) * 8
    ts = []
    for rep in range(5):
        t0 = time.perf_counter()
        sp = s.plane_spectra()
        ts.append((time.perf_counter() - t0) * 1e3)
    res["plane_spectra_ms"] = ts
    sets = {1: [40], 4: [0, 12, 40, 192], 16: [0, 4, 8, 12, 20, 40, 80, 120, 160, 192, 224, 264, 304, 344, 372, 384]}
    for rows, nf in (("velocity", 3), ("shear", 4)):
        res[f"ycross_{rows}_bytes_per_plane"] = (5 if s.combine() else nf) * field
        for n, refs in sets.items():
            ts = []
            for rep in range(5):
                t0 = time.perf_counter()
                cs = s.plane_cross_spectra(refs, rows)
                ts.append((time.perf_counter() - t0) * 1e3)
            tt = [s.plane_cross_spectra_timing(refs, rows) for _ in range(5)]
            key = f"ycross_{rows}_{n}"
            res[key + "_ms"] = ts
            res[key + "_over_step"] = min(ts) / step_ms
            res[key + "_kernel_ms"] = [t[0] for t in tt]
            res[key + "_kernel_ms_per_plane"] = min(t[0] for t in tt) / n
            res[key + "_yspectra_kernel_ms"] = [t[1] for t in tt]
            res[key + "_kernel_per_plane_over_yspectra"] = res[key + "_kernel_ms_per_plane"] / min(t[1] for t in tt)
            res[key + "_TBps"] = n * res[f"ycross_{rows}_bytes_per_plane"] / (min(t[0] for t in tt) * 1e-3) / 1e12
        if rows == "velocity":  # consistency: y = y_r against plane_spectra()
            own = cs["ckx"][0][9, 192].real
            res["ycross_uu_own_plane_vs_plane_spectra"] = float(abs(own - sp["ekx"][0][192]).max() / abs(sp["ekx"][0]).max())


if "--ycross-only" in sys.argv:
    cross_spectra_cost()
    print(json.dumps(res))
    sys.exit(0)
if "--sbudget-only" in sys.argv:
    spectral_budget_cost()
    print(json.dumps(res))
    sys.exit(0)
for rep in range(2):
    t0 = time.perf_counter()
    m = s.plane_moments()
    res[f"plane_moments_ms_{rep}"] = (time.perf_counter() - t0) * 1e3
# plane_histograms over every plane, without and with the vorticity: the whole call with the default
# centres and half-widths (one plane_moments() pass more for the r.m.s.; with the vorticity also one
# gradient_sums()), and the histogram pass alone with given ones, as every sample after the first of
# sample_statistics(pdfs=True) runs it; host time of the whole call (memset, launches, the 16 MB copy of the
# counts and their gathering included).  CHANNEL_HIST_MERGE=0: one LDS atomic per sample (A/B).
planes = list(range(cfg.NY))
for name, vort in (("plane_histograms", False), ("plane_histograms_vorticity", True)):
    ts = []
    for rep in range(3):
        t0 = time.perf_counter()
        h = s.plane_histograms(planes, vorticity=vort)
        ts.append((time.perf_counter() - t0) * 1e3)
    res[name + "_default_ms"] = ts
    c, hw = [float(v) for v in h["centre"].ravel()], [float(v) for v in h["halfwidth"].ravel()]
    for merge in ("1", "0"):
        os.environ["CHANNEL_HIST_MERGE"] = merge
        ts = []
        for rep in range(5):
            t0 = time.perf_counter()
            h = s.plane_histograms(planes, vorticity=vort, centre=c, halfwidth=hw)
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name + ("_ms" if merge == "1" else "_nomerge_ms")] = ts
    del os.environ["CHANNEL_HIST_MERGE"]
    res[name + "_over_step"] = min(res[name + "_ms"]) / step_ms
    res[name + "_over_plane_moments"] = min(res[name + "_ms"]) / res["plane_moments_ms_1"]
    res[name + "_out_of_range"] = float((h["hist"][:, :, 0] + h["hist"][:, :, -1]).sum() / h["hist"].sum())
res["plane_histograms_6_over_3"] = min(res["plane_histograms_vorticity_ms"]) / min(res["plane_histograms_ms"])
if "--pdfs-only" in sys.argv:
    print(json.dumps(res))
    sys.exit(0)
# gradient_sums: the six spectral fields read once (planes y < NY of the padded kz line stride),
# host time of the whole call (launches, the 21 KB result copy and its synchronisation included)
nkx, nkz = 2 * (cfg.NX // 3) + 1, (2 * cfg.NZ - 2) // 3 + 1
nkzs = (nkz + 7) // 8 * 8 if s.spec_kzb() else nkz
res["gradient_sums_bytes"] = 6 * cfg.NY * nkx * nkzs * 8
for name, call in (("gradient_sums", s.gradient_sums), ("transport_moments", s.transport_moments)):
    ts = []
    for rep in range(5):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    res[name + "_ms"] = ts
    res[name + "_over_step"] = min(ts) / step_ms
res["gradient_sums_TBps"] = res["gradient_sums_bytes"] / (min(res["gradient_sums_ms"]) * 1e-3) / 1e12
res["gradient_sums_over_floor_5p3TBps"] = min(res["gradient_sums_ms"]) * 1e-3 / (res["gradient_sums_bytes"] / 5.3e12)
# pressure: device time of the transform stage and of the y-line Poisson kernel (hipEvents), the
# kernel against its streaming floor of four field passes (three reads, one write) at 5.3 TB/s
res["pressure_solve_bytes"] = 4 * cfg.NY * nkx * nkzs * 8
tt = [s.pressure_timing() for _ in range(5)]
res["pressure_transforms_ms"] = [t[0] for t in tt]
res["pressure_solve_ms"] = [t[1] for t in tt]
res["pressure_hat_device_ms"] = min(t[0] + t[1] for t in tt)
res["pressure_hat_device_over_step"] = res["pressure_hat_device_ms"] / step_ms
res["pressure_solve_floor_over_time_5p3TBps"] = (res["pressure_solve_bytes"] / 5.3e12) / (min(res["pressure_solve_ms"]) * 1e-3)
ts = []
for rep in range(5):
    t0 = time.perf_counter()
    pm = s.pressure_moments()
    ts.append((time.perf_counter() - t0) * 1e3)
res["pressure_moments_ms"] = ts
res["pressure_moments_over_step"] = min(ts) / step_ms
res["p_rms_centre"] = float(pm[0, 192] ** 0.5)
# pressure strain: the solve, the export pass with the return trip of p' (one more single-field x-forward
# per chunk) and the Parseval pass over p-hat' and the four (combine mode: five) fields it reads; host time
# of the whole call (the device work, its launches, the 21 KB result copy and its synchronisation)
ts = []
for rep in range(5):
    t0 = time.perf_counter()
    ps = s.pressure_strain()
    ts.append((time.perf_counter() - t0) * 1e3)
res["pressure_strain_ms"] = ts
res["pressure_strain_over_step"] = min(ts) / step_ms
res["pressure_strain_over_pressure_moments"] = min(ts) / min(res["pressure_moments_ms"])
res["pstrain_trace_over_max"] = float(abs(ps[0] + ps[1] + ps[2]).max() / abs(ps[:3]).max())
res["pu_pstrain_vs_moments"] = float(abs(ps[4] - pm[1]).max() / abs(pm[1]).max())
# plane spectra: the read of gradient_sums() with a sum per (plane, |kx|) and (plane, kz); host time of the
# whole call (the 16.8 MB memset, the launch, the 16.8 MB result copy and its synchronisation), without and
# with the pressure row (then the device part of static_pressure_hat() first and a seventh field read)
res["plane_spectra_result_bytes"] = 8 * cfg.NY * (cfg.NX // 3 + 1 + nkz) * 8
for name, flag in (("plane_spectra", False), ("plane_spectra_pressure", True)):
    ts = []
    for rep in range(5):
        t0 = time.perf_counter()
        sp = s.plane_spectra(flag)
        ts.append((time.perf_counter() - t0) * 1e3)
    res[name + "_ms"] = ts
    res[name + "_over_step"] = min(ts) / step_ms
    res[name + "_over_gradient_sums"] = min(ts) / min(res["gradient_sums_ms"])
g = s.gradient_sums()
res["plane_spectra_wxwx_sum_vs_gradient_sums"] = float(abs(sp["ekx"][4].sum(axis=-1) - g[0]).max() / abs(g[0]).max())
res["plane_spectra_pp_sum_vs_pstrain"] = float(abs(sp["ekz"][7].sum(axis=-1) - ps[6]).max() / abs(ps[6]).max())
spectral_budget_cost()
if "--skip-fields" in sys.argv:
    print(json.dumps(res))
    sys.exit(0)
t0 = time.perf_counter()
f = s.physical_fields([192], ["u", "v", "w"])
res["physical_fields_1plane_ms"] = (time.perf_counter() - t0) * 1e3
del f
t0 = time.perf_counter()
f = s.physical_fields(list(range(385)), ["u", "v", "w"])
res["physical_fields_3x385_ms"] = (time.perf_counter() - t0) * 1e3
res["moments_over_step"] = res["plane_moments_ms_1"] / step_ms
res["fields_over_step"] = res["physical_fields_3x385_ms"] / step_ms
res["skew_u_centre"] = float(m[5, 192] / m[1, 192] ** 1.5)
res["u_shape"] = list(f["u"].shape)
print(json.dumps(res))
