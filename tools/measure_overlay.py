#!/usr/bin/env python3
"""Times atmrt_draw_overlay_device (README tick block, both lines on: FlatDistorted earth with refraction) on Fast frames of
4096 x 2048 and 8192 x 4096, beside atmrt_draw_image_device on the same frame (the project's memory-bound yardstick) and what a
host had to do before the overlay existed: download the elevation plane and scan it with numpy (tests/overlay_model.py).

    python tools/measure_overlay.py --out profiles/overlay.json            # wall clock around calls that end in a device synchronise
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure_overlay.py --calls 20 --size 4096x2048   # kernel times

Calls are timed after warm-up, repeated, and reported as median with minimum and maximum (milliseconds)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from atm_raytracer_amd import _lib, config, generators, synth  # noqa: E402

README_TICKS = [("Multiple", 0.0, 10.0, 10, True), ("Multiple", 0.0, 2.0, 5, False), ("Single", 45.0, 15, True)]
SCENES = {"4096x2048": "headline", "8192x4096": "S4"}


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def frame(ctx, size):
    import torch
    cfg, tiles = synth.scene(SCENES[size], generator="Fast", earth_shape="FlatDistorted")
    cfg.coloring = config._coloring({})
    w, h = cfg.params.width, cfg.params.height
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    planes, pod = generators.image_planes(h, w, torch.device("cuda", 0))
    gen.generate_device(pod)
    return cfg, planes, w, h


def measure(ctx, size, warmup, repeats, host_repeats):
    import torch
    import overlay_model as om
    cfg, planes, w, h = frame(ctx, size)
    col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    overlay = generators.into_overlay({"ticks": README_TICKS, "vertical_ticks": [], "show_eye_level": True, "show_flat_horizon": True})
    lines_only = generators.into_overlay({"show_eye_level": True, "show_flat_horizon": True})
    deg = C.c_double()

    def draw_image():
        ctx.check(ctx.lib.atmrt_draw_image_device(ctx.handle, C.byref(col), rgb.data_ptr()))

    def draw_overlay(o=overlay):
        ctx.check(ctx.lib.atmrt_draw_overlay_device(ctx.handle, C.byref(o), rgb.data_ptr(), None, 0, None, C.byref(deg)))

    out = {"width": w, "height": h, "elevation_plane_bytes": w * h * 8,
           "draw_image_device_call": timed(draw_image, warmup, repeats),
           "draw_overlay_device_call": timed(draw_overlay, warmup, repeats),
           "draw_overlay_device_call_lines_only": timed(lambda: draw_overlay(lines_only), warmup, repeats)}
    out["flat_horizon_deg"] = deg.value
    # before: the plane to the host (pageable memory, as a numpy caller gets it) + the sequential-in-y scan of the model, two targets
    host = {}
    host["download"] = timed(lambda: planes["elevation_angle"].cpu(), 1, host_repeats)
    el = planes["elevation_angle"].cpu().numpy()
    host["numpy_find_elev_two_targets"] = timed(lambda: (om.find_elev_all(el, deg.value), om.find_elev_all(el, 0.0)), 0, host_repeats)
    out["host_before"] = host
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", action="append", choices=sorted(SCENES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="only make this many draw_image + draw_overlay calls (for a profiler)")
    a = ap.parse_args()
    ctx = generators.Context(0)
    sizes = a.size or sorted(SCENES)
    if a.calls:
        import torch
        for size in sizes:
            cfg, planes, w, h = frame(ctx, size)
            col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
            rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            overlay = generators.into_overlay({"ticks": README_TICKS, "vertical_ticks": [], "show_eye_level": True, "show_flat_horizon": True})
            for _ in range(a.calls):
                ctx.check(ctx.lib.atmrt_draw_image_device(ctx.handle, C.byref(col), rgb.data_ptr()))
                ctx.check(ctx.lib.atmrt_draw_overlay_device(ctx.handle, C.byref(overlay), rgb.data_ptr(), None, 0, None, None))
        return 0
    result = {"source_hash": _lib.source_hash(), "method": "host clock around calls that end in a device synchronise; median of repeats after warm-up",
              "sizes": {size: measure(ctx, size, a.warmup, a.repeats, a.host_repeats) for size in sizes}}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
