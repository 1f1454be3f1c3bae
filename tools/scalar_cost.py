"""Cost of the passive scalar at 1024x385x1024 fp32 on one GPU.

Scalar off: ms/step of this tree against another checkout (--parent ROOT: a built tree of the parent commit),
in alternating rounds of fresh processes on one box; `scalar = false` changes no launch, so the two must
agree within the run-to-run spread of those same rounds, which is reported beside them.
Scalar on: ms/step, and the device time per substep of the flux pass (x-backward, zscalar, x-forward) and of
scalar_kernel by events (Solver.scalar_timing), next to the pressure solve's kernel for comparison.

Writes profiles/scalar/README.md and profiles/scalar/scalar_cost.json (--out DIR to change the place).
--grid NX NY NZ for a smaller grid; --rounds N alternating rounds (default 3)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    """One fresh process: steps of one tree, scalar on or off; prints one JSON line."""
    sys.path.insert(0, a.tree)
    from channel_gpu_amd import require_core
    from channel_gpu_amd.utils.config import default_config

    C = require_core()
    kw = dict(NX=a.grid[0], NY=a.grid[1], NZ=a.grid[2], Re=20700.0, precision="fp32", ic="random", ic_amplitude=0.05,
              stats_every=0, log_every=0, symmetry_every=0)
    if a.scalar:
        kw.update(scalar=True, Pr=0.71, scalar_lower=-1.0, scalar_upper=1.0)
    s = C.Solver(default_config(**kw), 0, 1, 0, b"")
    s.init_ic()
    s.prepare()
    for _ in range(a.warmup):
        s.step(False)
    s.synchronize()
    s.set_step_timing(True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        s.step(False)
    s.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / a.steps
    dev = list(s.step_times_ms())
    out = {"tree": a.tree, "scalar": bool(a.scalar), "wall_ms_per_step": wall, "device_ms_per_step_median": statistics.median(dev),
           "device_ms_per_step_min": min(dev), "graph": bool(s.graph_active()), "health": int(s.health())}
    if a.scalar:
        tt = [s.scalar_timing() for _ in range(5)]
        for i, k in enumerate(("xbackward", "zscalar", "xforward", "scalar_kernel")):
            out[f"substep_{k}_ms"] = [t[i] for t in tt]
        out["pressure_solve_kernel_ms"] = [s.pressure_timing()[1] for _ in range(5)]
    print(json.dumps(out), flush=True)


def run_child(tree, scalar, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--grid", *map(str, a.grid)] + (["--scalar"] if scalar else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}): {' '.join(cmd)}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--scalar", action="store_true")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (scalar off A/B)")
    ap.add_argument("--grid", type=int, nargs=3, default=[1024, 385, 513])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"grid": "x".join(map(str, (a.grid[0], a.grid[1], 2 * a.grid[2] - 2))), "precision": "fp32", "steps": a.steps,
           "warmup": a.warmup, "rounds": []}
    for r in range(a.rounds):  # alternating: this tree, the parent, this tree with the scalar
        rnd = {"this_off": run_child(ROOT, False, a)}
        if a.parent:
            rnd["parent_off"] = run_child(os.path.abspath(a.parent), False, a)
        rnd["this_on"] = run_child(ROOT, True, a)
        res["rounds"].append(rnd)
    col = lambda k, f="device_ms_per_step_median": [x[k][f] for x in res["rounds"] if k in x]  # noqa: E731
    summ = {}
    for k in ("this_off", "parent_off", "this_on"):
        v = col(k)
        if v:
            summ[k] = {"ms_per_step": v, "median": statistics.median(v), "spread": max(v) - min(v)}
    res["summary"] = summ
    on = [x["this_on"] for x in res["rounds"]]
    for k in ("xbackward", "zscalar", "xforward", "scalar_kernel"):
        summ[f"substep_{k}_ms"] = min(min(o[f"substep_{k}_ms"]) for o in on)
    summ["pressure_solve_kernel_ms"] = min(min(o["pressure_solve_kernel_ms"]) for o in on)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scalar_cost.json"), "w") as f:
        json.dump(res, f, indent=1)
    L = [f"# Cost of the passive scalar, {res['grid']} fp32, one GPU", "",
         f"`tools/scalar_cost.py`: {a.rounds} alternating rounds of fresh processes, {a.warmup} warm-up and {a.steps} timed steps each;",
         "ms/step is the median of the per-step device times (events around every step), the spread is max - min over the rounds.", "",
         "| run | ms/step per round | median | spread |", "|---|---|---|---|"]
    names = {"this_off": "this tree, scalar off", "parent_off": "parent commit", "this_on": "this tree, scalar on"}
    for k, v in summ.items():
        if isinstance(v, dict):
            L.append(f"| {names[k]} | {', '.join(f'{x:.3f}' for x in v['ms_per_step'])} | {v['median']:.3f} | {v['spread']:.3f} |")
    if "parent_off" in summ:
        d = summ["this_off"]["median"] - summ["parent_off"]["median"]
        sp = max(summ["this_off"]["spread"], summ["parent_off"]["spread"])
        L += ["", f"Scalar off against the parent: {d:+.3f} ms/step, run-to-run spread in these rounds {sp:.3f} ms/step."]
    add = summ["this_on"]["median"] - summ["this_off"]["median"]
    fl = sum(summ[f"substep_{k}_ms"] for k in ("xbackward", "zscalar", "xforward"))
    L += ["", f"Scalar on adds {add:.3f} ms/step ({100 * add / summ['this_off']['median']:.1f} %).", "",
          "Device time per substep of the scalar's stages (events, the stages serialised on one stream; best of 5 x rounds):", "",
          "| stage | ms per substep |", "|---|---|"]
    for k, n in (("xbackward", "x-backward of u, v, w and theta"), ("zscalar", "zscalar"), ("xforward", "x-forward of the three fluxes"),
                 ("scalar_kernel", "scalar_kernel")):
        L.append(f"| {n} | {summ[f'substep_{k}_ms']:.3f} |")
    L += [f"| flux pass in all | {fl:.3f} |", f"| (the pressure solve's y-line kernel, for comparison) | {summ['pressure_solve_kernel_ms']:.3f} |", ""]
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(L))
    print(json.dumps(summ))


if __name__ == "__main__":
    main()
