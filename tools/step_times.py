#!/usr/bin/env python3
"""Per-step device times of the headline benchmark, with the statistics steps marked.

Same set-up as bench.py (same configuration, torch-free, step graph on, plane statistics every
``--stats-every``-th timed step), but instead of the median and p90 it prints every per-step
device time that ``Solver.step_times_ms()`` holds: the wall mean that bench.py's ``value`` is
computed from pays for the statistics steps in full, the median never contains them.

  python tools/step_times.py [--steps 20] [--warmup 5] [--grid 1024x385x1024] [--stats-every 10]

Prints one line per step and one JSON summary line (plain mean, statistics mean, their difference).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", default="1024x385x1024", help="NX x NY x Nz_physical")
    ap.add_argument("--re", type=float, default=20700.0)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--stats-every", type=int, default=10)
    args = ap.parse_args()

    os.environ["CHANNEL_TORCH_FREE"] = "1"
    from channel_gpu_amd import require_core
    from channel_gpu_amd.parallel.native_bootstrap import init_native
    from channel_gpu_amd.utils.config import default_config

    ri = init_native()
    C = require_core()
    NX, NY, NZP = (int(v) for v in args.grid.lower().split("x"))
    cfg = default_config(NX=NX, NY=NY, NZ=NZP // 2 + 1, Re=args.re, precision=args.precision, ic="random",
                         ic_amplitude=0.05, stats_every=0, log_every=0, symmetry_every=0, checkpoint_every=0,
                         health_check=True)
    solver = C.Solver(cfg, ri.rank, ri.world, ri.device, ri.uid)
    solver.init_ic()
    solver.prepare()
    se = max(0, args.stats_every)
    for i in range(args.warmup):
        solver.step(se > 0 and args.warmup >= 2 and i == args.warmup - 1)
    solver.barrier()
    solver.set_step_timing(True)
    t0 = time.perf_counter()
    marks = []
    for i in range(args.steps):
        marks.append(se > 0 and (i + 1) % se == 0)
        solver.step(marks[-1])
    solver.barrier()
    wall_ms = 1e3 * (time.perf_counter() - t0) / max(1, args.steps)
    ms = list(solver.step_times_ms())
    solver.set_step_timing(False)
    for i, (t, m) in enumerate(zip(ms, marks)):
        print(f"step {i + 1:3d}  {t:8.3f} ms{'  statistics' if m else ''}")
    plain = [t for t, m in zip(ms, marks) if not m]
    stat = [t for t, m in zip(ms, marks) if m]
    mean = lambda v: sum(v) / len(v) if v else float("nan")  # noqa: E731
    print(json.dumps({"grid": args.grid, "steps": args.steps, "stats_every": se, "graph": bool(solver.graph_active()),
                      "wall_ms_per_step": round(wall_ms, 4), "plain_mean_ms": round(mean(plain), 4),
                      "plain_min_ms": round(min(plain), 4) if plain else None,
                      "plain_max_ms": round(max(plain), 4) if plain else None,
                      "stats_mean_ms": round(mean(stat), 4), "stats_minus_plain_ms": round(mean(stat) - mean(plain), 4)}),
          flush=True)
    del solver


if __name__ == "__main__":
    main()
