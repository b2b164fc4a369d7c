#!/usr/bin/env python3
"""Times atmrt_viewshed at the headline's setting (scene "headline": nine tiles, observer 500 m above the ground, refraction on,
step 100 m) on the headline's lattice: 4096 azimuths over the full circle x 2000 samples (200 km), a fan of 1024 rays over
-5 .. 5 degrees, height 0, all seven planes downloaded.  The library reports where the time of a call went
(atmrt_last_viewshed_timings: path table, profiles, scan and download between events on its stream); the whole synchronous call is
timed on the host clock besides.  The path table is kept across calls, so its time comes from calls whose fan is nudged by one ulp
(a rebuild each); the other three phases from calls that find the table.

The parent of the change that added the viewshed has one route to the same cells: atmrt_sight_lines(rounds = 1), at most 65,536
targets per call.  It is timed on the first 65,536 cells of the same lattice (azimuth-major: the first 32 azimuths and part of the
33rd, every distance from 100 m to 200 km) with a 64-ray fan — its only fan — and reported as cells per second beside the viewshed's.

    python tools/measure_viewshed.py --out profiles/viewshed.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from atm_raytracer_amd import _lib, generators, synth  # noqa: E402


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rebuilds", type=int, default=3)
    ap.add_argument("--azimuths", type=int, default=4096)
    ap.add_argument("--reach", type=float, default=200_000.0)
    ap.add_argument("--fan-rays", type=int, default=1024)
    ap.add_argument("--sight-cells", type=int, default=65536)
    a = ap.parse_args()
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", generator="Fast")
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))._configure()
    fan, az_step = (-5.0, 5.0), 360.0 / a.azimuths
    shape = generators.viewshed_kernel_shape(a.fan_rays)
    result = {"source_hash": _lib.source_hash(), "azimuths": a.azimuths, "reach_m": a.reach, "simulation_step_m": cfg.params.simulation_step,
              "fan_deg": list(fan), "fan_rays": a.fan_rays, "kernel_shape": shape,
              "method": "per call: atmrt_last_viewshed_timings (path table, profiles with their upload, scan, download between events on the "
                        "library's stream, the last three summed over the call's batches) and the host clock around the whole synchronous call; "
                        "median of repeats after warm-up; the path table's time from calls whose fan_hi is nudged by one ulp",
              "parent_commit": "no viewshed: its only route to these cells is atmrt_sight_lines(rounds = 1), timed below on the first cells of the lattice"}
    parts, calls = {}, []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        v = generators.viewshed(ctx, 0.0, az_step, a.azimuths, a.reach, 0.0, fan, a.fan_rays)
        calls.append((time.perf_counter() - t0) * 1e3)
        if i >= a.warmup:
            for k, val in generators.viewshed_work(ctx).items():
                parts.setdefault(k, []).append(val)
    n_az, m = v.k_star.shape
    cells = n_az * m
    assert not any(parts.pop("table_rebuilt")), "a call with the same fan must find the path table"
    batches = parts.pop("batches")[0]
    parts.pop("paths_ms")
    rebuilds, hi = [], fan[1]
    for _ in range(a.rebuilds):
        hi = float(np.nextafter(hi, 10.0))
        generators.viewshed(ctx, 0.0, az_step, 1, a.reach, 0.0, (fan[0], hi), a.fan_rays, optional=())
        w = generators.viewshed_work(ctx)
        assert w["table_rebuilt"]
        rebuilds.append(w["paths_ms"])
    device_ms = statistics.median(parts["profiles_ms"]) + statistics.median(parts["scan_ms"])
    result["viewshed"] = {"cells": cells, "samples_per_azimuth": m, "batches": batches, "call_host_clock": spread(calls[a.warmup:]),
                          "paths_ms": spread(rebuilds), **{k: spread(val) for k, val in parts.items()},
                          "cells_per_second_profiles_and_scan": cells / (device_ms * 1e-3),
                          "cells_per_second_whole_call": cells / (statistics.median(calls[a.warmup:]) * 1e-3),
                          "status_counts_seen_hidden_above_below": np.bincount(v.status.ravel(), minlength=4).tolist()}
    # the parent's route: the first cells of the same lattice as sight-line targets
    n = min(a.sight_cells, cells, 65536)
    idx = np.arange(n)
    targets = np.zeros(n, dtype=generators.SIGHT_TARGET_DTYPE)
    targets["azimuth_deg"], targets["distance"] = v.azimuths[idx // m], v.d[1 + idx % m]
    sparts, scalls = {}, []
    for i in range(a.warmup + max(a.repeats // 2, 1)):
        t0 = time.perf_counter()
        s = generators.sight_lines(ctx, targets, fan, 1)
        scalls.append((time.perf_counter() - t0) * 1e3)
        if i >= a.warmup:
            for k, val in generators.sight_timings(ctx).items():
                sparts.setdefault(k, []).append(val)
    sb = sparts.pop("batches")[0]
    sdev = statistics.median(sparts["profile_ms"]) + statistics.median(sparts["solve_ms"])
    result["sight_lines_rounds_1"] = {"cells": n, "fan_rays": 64, "batches": sb, "call_host_clock": spread(scalls[a.warmup:]),
                                      **{k: spread(val) for k, val in sparts.items()},
                                      "cells_per_second_profile_and_solve": n / (sdev * 1e-3),
                                      "cells_per_second_whole_call": n / (statistics.median(scalls[a.warmup:]) * 1e-3),
                                      "status_counts_seen_hidden_above_below": np.bincount(s["status"], minlength=4).tolist()}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
