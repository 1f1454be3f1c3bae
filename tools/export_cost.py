"""Cost of one plane_moments() and one three-field all-plane physical_fields() at 1024x385x1024 fp32,
relative to one RK3 step on the same box."""
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
for rep in range(2):
    t0 = time.perf_counter()
    m = s.plane_moments()
    res[f"plane_moments_ms_{rep}"] = (time.perf_counter() - t0) * 1e3
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
