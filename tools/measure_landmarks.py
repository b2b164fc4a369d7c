#!/usr/bin/env python3
"""Times atmrt_locate_landmarks on the headline frame (4096 x 2048, Fast and Rectilinear, left in HBM by atmrt_generate_device) for
1,000 and 50,000 landmarks drawn uniformly over the frame's bounds, radius 3 arcseconds, FIRST and ALL mode.  The library reports
where the time of a call went (atmrt_last_landmark_timings): the host's index build, the upload of the index, and the three
passes between events on its stream; the whole synchronous call is timed on the host clock besides.  Beside them: the
visibility-map scatter of the same frame at 3-arcsecond cells (the same reads: the natural yardstick).

    python tools/measure_landmarks.py --out profiles/landmarks.json

Per case the landmarks' n_within are summarised (how many found, the largest, their sum): where a few landmarks collect thousands of
points, their two atomic addresses are what passes A and B wait for."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from atm_raytracer_amd import _abi, _lib, generators, synth  # noqa: E402

RADIUS = 3.0 / 3600.0


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--generators", default="Fast,Rectilinear")
    ap.add_argument("--counts", default="1000,50000")
    a = ap.parse_args()
    import torch
    ctx = generators.Context(0)
    result = {"source_hash": _lib.source_hash(), "radius_arcsec": 3.0,
              "method": "per call: atmrt_last_landmark_timings (index build on the host clock; upload + reset, pass A, pass B, pass C between "
                        "events on the library's stream) and the host clock around the whole synchronous call; median of repeats after warm-up",
              "frames": {}}
    rng = np.random.default_rng(1)
    for gen_name in a.generators.split(","):
        cfg, tiles = synth.scene("headline", generator=gen_name)
        w, h = cfg.params.width, cfg.params.height
        gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
        planes, pod = generators.image_planes(h, w, torch.device("cuda", 0))
        _, frame_ms = gen.generate_device(pod)
        frame = {"width": w, "height": h, "generate_device_ms": frame_ms, "cases": {}}
        for mode in ("first", "all"):
            bounds = generators.frame_bounds(ctx, mode)
            grid = generators.snap_grid(bounds, RADIUS)
            count = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.int32, device="cuda")
            mind = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.float64, device="cuda")
            st = _abi.VisibilityStats()

            def vis_map():
                ctx.check(ctx.lib.atmrt_visibility_map_device(ctx.handle, C.byref(grid), _abi.VIS_MODES[mode], count.data_ptr(), mind.data_ptr(), C.byref(st)))

            ms = []
            for i in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                vis_map()
                ms.append((time.perf_counter() - t0) * 1e3)
            frame["cases"][f"visibility_map_3as_{mode}"] = {"call_host_clock": spread(ms[a.warmup:]), "cells": grid.n_lat * grid.n_lon,
                                                            **{k: getattr(st, k) for k, _ in _abi.VisibilityStats._fields_}}
            for n in (int(x) for x in a.counts.split(",")):
                marks = generators.landmarks(rng.uniform(bounds[0], bounds[1], n), rng.uniform(bounds[2], bounds[3], n))
                parts, calls = {}, []
                for i in range(a.warmup + a.repeats):
                    t0 = time.perf_counter()
                    hits, stats = generators.locate_landmarks(ctx, marks, RADIUS, mode)
                    calls.append((time.perf_counter() - t0) * 1e3)
                    if i >= a.warmup:
                        for k, v in generators.landmark_timings(ctx).items():
                            parts.setdefault(k, []).append(v)
                nw = hits["n_within"].astype(np.int64)
                frame["cases"][f"landmarks_{n}_{mode}"] = {
                    "call_host_clock": spread(calls[a.warmup:]), **{k: spread(v) for k, v in parts.items()}, **stats,
                    "found": int((nw > 0).sum()), "largest_n_within": int(nw.max()), "landmarks_with_over_1000_within": int((nw > 1000).sum()),
                    "n_within_percentiles_of_found": [int(x) for x in np.percentile(nw[nw > 0], [50, 90, 99, 100])] if (nw > 0).any() else []}
        result["frames"][gen_name] = frame
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
