"""Cost of a restart onto another grid on one MI355X: a 512x257x512 fp32 state (written by a source
solver into a temporary directory) is loaded with `regrid` into 1024x385x1024 fp32.  Reported separately:
the HDF5 read, the upload, the regrid kernel and the whole call, and the kernel's bytes moved over its
time next to the 5.3 TB/s streaming rate.  For comparison, on the same box: a plain same-grid
read_restart of a 1024x385x1024 file (written from the regridded state), which runs the host unpack and
set_state.  One JSON line on stdout; --out also writes it to a file.

    python tools/regrid_cost.py [--src 512 257 257] [--dst 1024 385 513] [--out FILE] [--tmp DIR] [--skip-plain]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from channel_gpu_amd import require_core  # noqa: E402
from channel_gpu_amd.utils.config import default_config  # noqa: E402

STREAM_TBPS = 5.3


def note(msg):
    print(f"[regrid_cost] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, nargs=3, default=[512, 257, 257], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--dst", type=int, nargs=3, default=[1024, 385, 513], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--out", default="")
    ap.add_argument("--tmp", default=None, help="directory for the temporary restart files")
    ap.add_argument("--skip-plain", action="store_true", help="leave the same-grid baseline out")
    a = ap.parse_args()
    C = require_core()
    kw = dict(Re=20700.0, precision=a.precision, stats_every=0, log_every=0, symmetry_every=0)
    res = {"source": "x".join(map(str, a.src)), "target": "x".join(map(str, a.dst)), "precision": a.precision}
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        g, ddv = os.path.join(d, "G.h5"), os.path.join(d, "DDV.h5")
        src = C.Solver(default_config(NX=a.src[0], NY=a.src[1], NZ=a.src[2], ic="random", ic_amplitude=0.05, **kw), 0, 1, 0, b"")
        src.init_ic()
        t0 = time.perf_counter()
        src.write_restart(g, ddv, "-")
        res["source_write_s"] = time.perf_counter() - t0
        del src
        note(f"source files written in {res['source_write_s']:.1f} s")

        dst = C.Solver(default_config(NX=a.dst[0], NY=a.dst[1], NZ=a.dst[2], ic="zero", regrid=True, **kw), 0, 1, 0, b"")
        runs = []
        for rep in range(2):  # (the first call also pays the page cache and the allocator)
            t0 = time.perf_counter()
            dst.read_restart(g, ddv, "-")
            wall = time.perf_counter() - t0
            read, upload, kernel, total = dst.regrid_timing()
            runs.append(dict(wall_s=wall, read_ms=read, upload_ms=upload, kernel_ms=kernel, total_ms=total))
            note(f"regrid {rep}: {runs[-1]}")
        res["regrid_runs"] = runs
        best = min(runs, key=lambda r: r["total_ms"])
        res["regrid"] = best
        # bytes the kernel moves at least: every staged source line once (fp64 complex), every target element once
        esz = 16 if a.precision == "fp64" else 8
        nkx_d, nkz_d = 2 * (a.dst[0] // 3) + 1, (2 * a.dst[2] - 2) // 3 + 1
        nkx_t = min(nkx_d, 2 * (a.src[0] // 3) + 1)
        nkz_t = min(nkz_d, (2 * a.src[2] - 2) // 3 + 1)
        nkzs = (nkz_d + 7) // 8 * 8 if dst.spec_kzb() else nkz_d
        rd = 2 * nkx_t * nkz_t * a.src[1] * 16
        wr = 2 * nkx_t * ((nkz_t + 7) // 8 * 8) * a.dst[1] * esz
        zero = 4 * ((a.dst[1] + 7) // 8 * 8 if dst.spec_kzb() else a.dst[1]) * nkx_d * nkzs * esz
        res["kernel_bytes"] = dict(staged_read=rd, tile_write=wr, memset_not_in_kernel_time=zero)
        res["kernel_TBps"] = (rd + wr) / (best["kernel_ms"] * 1e-3) / 1e12
        res["kernel_over_streaming_rate"] = res["kernel_TBps"] / STREAM_TBPS
        res["kernel_share_of_total"] = best["kernel_ms"] / best["total_ms"]
        res["health_after_regrid"] = int(dst.health())

        if not a.skip_plain:
            g2, ddv2 = os.path.join(d, "G2.h5"), os.path.join(d, "DDV2.h5")
            t0 = time.perf_counter()
            dst.write_restart(g2, ddv2, "-")
            res["target_write_s"] = time.perf_counter() - t0
            note(f"target files written in {res['target_write_s']:.1f} s")
            del dst
            plain = C.Solver(default_config(NX=a.dst[0], NY=a.dst[1], NZ=a.dst[2], ic="zero", **kw), 0, 1, 0, b"")
            ts = []
            for rep in range(2):
                t0 = time.perf_counter()
                plain.read_restart(g2, ddv2, "-")
                ts.append(time.perf_counter() - t0)
                note(f"plain same-grid read_restart {rep}: {ts[-1]:.2f} s")
            res["plain_same_grid_read_restart_s"] = ts
            # the same files through the regrid path (identity: unit rows), on the same box
            same = C.Solver(default_config(NX=a.dst[0], NY=a.dst[1], NZ=a.dst[2], ic="zero", regrid=True, **kw), 0, 1, 0, b"")
            t0 = time.perf_counter()
            same.read_restart(g2, ddv2, "-")
            res["regrid_same_grid_s"] = time.perf_counter() - t0
            read, upload, kernel, total = same.regrid_timing()
            res["regrid_same_grid"] = dict(read_ms=read, upload_ms=upload, kernel_ms=kernel, total_ms=total)
            note(f"same-grid files through the regrid path: {res['regrid_same_grid_s']:.2f} s")
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
