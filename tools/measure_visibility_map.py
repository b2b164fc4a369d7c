#!/usr/bin/env python3
"""Times atmrt_visibility_map_device on the headline frame (Fast, 4096 x 2048, left in HBM by atmrt_generate_device) for three grids
over the frame's bounds — 3 arcseconds, 30 arcseconds, one cell — with the wavefront aggregation on and off
(ATMRT_VIS_AGGREGATE), beside atmrt_draw_image_device on the same frame: the project's yardstick for one pass over the planes.

    python tools/measure_visibility_map.py --out profiles/visibility_map.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure_visibility_map.py --calls 20      # kernel times

A call launches on the library's own stream and ends in a synchronise of it, so the events (torch.cuda.Event pairs recorded on
the idle default stream right before and after the call) and the host clock measure the same thing: the whole call — the reset of
the statistics block, the clear of the map (12 B per cell), the scatter, the read-back of 72 B.  Both are reported, as median,
minimum and maximum over the repeats after warm-up, the two aggregation modes alternating call by call."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from atm_raytracer_amd import _abi, _lib, config, generators, synth  # noqa: E402

CELLS_ARCSEC = {"3as": 3.0, "30as": 30.0}


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def timed_call(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--calls", type=int, default=0, help="only make this many calls per grid and mode (for a profiler)")
    a = ap.parse_args()
    import torch
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", generator="Fast")
    cfg.coloring = config._coloring({})
    w, h = cfg.params.width, cfg.params.height
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    planes, pod = generators.image_planes(h, w, torch.device("cuda", 0))
    _, frame_ms = gen.generate_device(pod)
    bounds = generators.frame_bounds(ctx, "first")
    grids = {name: generators.snap_grid(bounds, sec / 3600.0) for name, sec in CELLS_ARCSEC.items()}
    grids["one"] = _abi.GeoGrid(-90.0, -180.0, 180.0, 360.0, 1, 1)
    col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    st = _abi.VisibilityStats()

    def draw_image():
        ctx.check(ctx.lib.atmrt_draw_image_device(ctx.handle, C.byref(col), rgb.data_ptr()))

    def run(fn, n):
        ev, host = zip(*[timed_call(fn) for _ in range(n)])
        return {"events": spread(ev), "host_clock": spread(host)}

    result = {"source_hash": _lib.source_hash(), "width": w, "height": h, "generate_device_ms": frame_ms, "bounds": list(bounds),
              "method": "whole synchronous call: torch.cuda.Event pair on the idle default stream around it, and the host clock; "
                        "median of repeats after warm-up, aggregate on / off alternating", "grids": {}}
    for _ in range(a.warmup):
        draw_image()
    if not a.calls:
        result["draw_image_device_call"] = run(draw_image, a.repeats)
    for name, grid in grids.items():
        count = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.int32, device="cuda")
        mind = torch.empty((grid.n_lat, grid.n_lon), dtype=torch.float64, device="cuda")

        def vis_map(aggregate):
            os.environ["ATMRT_VIS_AGGREGATE"] = "on" if aggregate else "off"
            ctx.check(ctx.lib.atmrt_visibility_map_device(ctx.handle, C.byref(grid), _abi.VIS_FIRST, count.data_ptr(), mind.data_ptr(), C.byref(st)))
            return {k: getattr(st, k) for k, _ in _abi.VisibilityStats._fields_}

        if a.calls:
            for _ in range(a.calls):
                vis_map(True), vis_map(False)
            continue
        for _ in range(a.warmup):
            vis_map(True), vis_map(False)
        times = {True: [], False: []}
        for _ in range(a.repeats):
            for aggregate in (True, False):
                times[aggregate].append(timed_call(lambda: vis_map(aggregate)))
        maps = {}
        entry = {"n_lat": grid.n_lat, "n_lon": grid.n_lon, "cells": grid.n_lat * grid.n_lon, "map_bytes": 12 * grid.n_lat * grid.n_lon}
        for aggregate in (True, False):
            stats = vis_map(aggregate)
            maps[aggregate] = (count.clone(), mind.clone())
            ev, host = zip(*times[aggregate])
            entry["aggregate_on" if aggregate else "aggregate_off"] = {"events": spread(ev), "host_clock": spread(host), **stats}
        entry["maps_identical"] = bool(torch.equal(maps[True][0], maps[False][0]) and torch.equal(maps[True][1], maps[False][1]))
        result["grids"][name] = entry
    os.environ.pop("ATMRT_VIS_AGGREGATE", None)
    if a.calls:
        return 0
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
