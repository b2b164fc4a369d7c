#!/usr/bin/env python3
"""Times atmrt_horizon at the headline's setting (scene "headline": nine tiles, observer 500 m above the ground, refraction on,
step 100 m) at the shape the viewshed is measured at (tools/measure_viewshed.py): 4096 azimuths over the full circle x 2000
samples (200 km), a first fan of 1024 rays over -5 .. 5 degrees.  For rounds = 1 and rounds = 3 the library reports where the time
of a call went (atmrt_last_horizon_timings: path table, profiles, scan, refine and download between events on its stream); the whole
synchronous call is timed on the host clock besides.  The path table is kept across calls, so its time comes from calls whose fan is
nudged by one ulp (a rebuild each); the other phases from calls that find the table.

In the same run the viewshed's scan is timed at the same shape (height 0, the three required planes only), as the figure beside the
horizon's: round one reads the same table against the same profiles, writes one record per azimuth instead of one per cell, and may
leave the step loop early.

    python tools/measure_horizon.py --out profiles/horizon.json"""
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
    a = ap.parse_args()
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", generator="Fast")
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))._configure()
    fan, az_step = (-5.0, 5.0), 360.0 / a.azimuths
    result = {"source_hash": _lib.source_hash(), "azimuths": a.azimuths, "reach_m": a.reach, "simulation_step_m": cfg.params.simulation_step,
              "fan_deg": list(fan), "fan_rays": a.fan_rays, "kernel_shape": generators.horizon_kernel_shape(a.fan_rays),
              "method": "per call: atmrt_last_horizon_timings (path table, profiles with their upload, scan, refine, download between events on the "
                        "library's stream, the last four summed over the call's batches) and the host clock around the whole synchronous call; "
                        "median of repeats after warm-up; the path table's time from calls whose fan_hi is nudged by one ulp; the viewshed's scan "
                        "from atmrt_last_viewshed_timings of calls at the same shape in the same run"}
    for rounds in (1, 3):
        parts, calls = {}, []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            h = generators.horizon(ctx, 0.0, az_step, a.azimuths, a.reach, fan, a.fan_rays, rounds)
            calls.append((time.perf_counter() - t0) * 1e3)
            if i >= a.warmup:
                for k, val in generators.horizon_work(ctx).items():
                    parts.setdefault(k, []).append(val)
        assert not any(parts.pop("table_rebuilt")), "a call with the same fan must find the path table"
        batches = parts.pop("batches")[0]
        parts.pop("paths_ms")
        rec = h.records
        found = rec["status"] == 0
        device_ms = sum(statistics.median(parts[k]) for k in ("profiles_ms", "scan_ms", "refine_ms"))
        result[f"rounds_{rounds}"] = {
            "batches": batches, "call_host_clock": spread(calls[a.warmup:]), **{k: spread(val) for k, val in parts.items()},
            "azimuths_per_second_profiles_scan_refine": a.azimuths / (device_ms * 1e-3),
            "azimuths_per_second_whole_call": a.azimuths / (statistics.median(calls[a.warmup:]) * 1e-3),
            "status_counts_found_-_above_below": np.bincount(rec["status"], minlength=4).tolist(),
            "rounds_done_counts": np.bincount(rec["rounds_done"], minlength=5).tolist(),
            "median_resolution_deg": float(np.median(rec["resolution"][found])) if found.any() else None,
            "median_ridge_distance_m": float(np.nanmedian(rec["block_distance"][found])) if found.any() else None}
    rebuilds, hi = [], fan[1]
    for _ in range(a.rebuilds):
        hi = float(np.nextafter(hi, 10.0))
        generators.horizon(ctx, 0.0, az_step, 1, a.reach, (fan[0], hi), a.fan_rays, 1)
        w = generators.horizon_work(ctx)
        assert w["table_rebuilt"]
        rebuilds.append(w["paths_ms"])
    result["paths_ms"] = spread(rebuilds)
    # the figure beside it: the viewshed's scan at the same shape
    vparts = {}
    for i in range(a.warmup + a.repeats):
        v = generators.viewshed(ctx, 0.0, az_step, a.azimuths, a.reach, 0.0, fan, a.fan_rays, optional=())
        if i >= a.warmup:
            for k, val in generators.viewshed_work(ctx).items():
                vparts.setdefault(k, []).append(val)
    result["viewshed_same_shape"] = {"cells": int(v.k_star.size), "batches": vparts["batches"][0], "scan_ms": spread(vparts["scan_ms"]),
                                     "profiles_ms": spread(vparts["profiles_ms"])}
    result["scan_ms_horizon_over_viewshed"] = result["rounds_1"]["scan_ms"]["median_ms"] / result["viewshed_same_shape"]["scan_ms"]["median_ms"]
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
