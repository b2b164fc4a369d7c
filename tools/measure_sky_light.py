#!/usr/bin/env python3
"""Times the sky light (include/atmrt.h, "sky light") beside the calls it extends, on the headline frame (scene "headline": nine
tiles, observer 500 m above the ground, refraction on, step 100 m, 4096 x 2048, Rectilinear) to a top of 100 km with the sky step at
100 m and at 1000 m:

  march   atmrt_sky_light_device (k_sky_light_march: the sky march with the refractivity column) against atmrt_sky_directions_device
          (k_sky_march) in the same process, both by atmrt_last_sky_timings' march interval, the calls alternating;
  shade   atmrt_sky_shade_device (k_sky_shade) against atmrt_sky_bodies_device (k_sky_bodies) with a sun and a moon in the frame, both
          by the host's clock around the call (the bodies call reports no time of its own), and the shade's kernel between events
          (atmrt_last_sky_shade_timing).

There is no pass threshold: the call runs once per frame.  Every figure is the median over --processes fresh processes of the median
over --repeats calls after --warmup calls.  ATMRT_LIB (atm_raytracer_amd._lib) names an experimental build of the library, e.g. one
with EXTRA=-DATMRT_SKY_LIGHT_WAVES_PER_EU=5.

    python tools/measure_sky_light.py --out profiles/sky_light.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

TOP, FLOOR = 100_000.0, 0.0
STEPS = (1000.0, 100.0)


def child(a):
    import torch
    from atm_raytracer_amd import _abi, generators, synth
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", a.width, a.height, generator="Rectilinear")
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    dev = torch.device("cuda", 0)
    planes, pod = generators.image_planes(a.height, a.width, dev)
    gen.generate_device(pod)
    shape = (a.height, a.width)
    true = torch.empty(shape, dtype=torch.float64, device=dev)
    column = torch.empty(shape, dtype=torch.float64, device=dev)
    status = torch.empty(shape, dtype=torch.uint8, device=dev)
    body = torch.empty(shape, dtype=torch.uint8, device=dev)
    rgb = torch.zeros(shape + (3,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    out = {}
    direction = float(cfg.params.frame.direction)
    bodies, n_bodies = generators._sky_bodies_array([(direction - 3.0, 0.2, generators.SUN_RADIUS_DEG, (255, 244, 214)),
                                                     (direction + 5.0, 4.0, generators.SUN_RADIUS_DEG, (226, 228, 235))])
    for step in STEPS:
        sky, light, st, z0 = generators.sky_spec(step, TOP, FLOOR), generators.sky_light_spec(0.0, step=step, top=TOP, floor=FLOOR), _abi.SkyStats(), C.c_double()
        parent, mine = [], []
        for i in range(a.warmup + a.repeats):
            ctx.check(ctx.lib.atmrt_sky_directions_device(ctx.handle, C.byref(sky), true.data_ptr(), status.data_ptr(), None, C.byref(st)))
            t_parent = generators.sky_timings(ctx)["march_ms"]
            ctx.check(ctx.lib.atmrt_sky_light_device(ctx.handle, C.byref(light), true.data_ptr(), status.data_ptr(), None, column.data_ptr(), C.byref(st),
                                                     C.byref(z0)))
            if i >= a.warmup:
                parent.append(t_parent)
                mine.append(generators.sky_timings(ctx)["march_ms"])
        stats = generators._sky_stats(st)
        shade = generators.sky_shade_params(z0.value)
        t_bodies, t_shade, t_kernel = [], [], []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            ctx.check(ctx.lib.atmrt_sky_bodies_device(ctx.handle, bodies, n_bodies, true.data_ptr(), status.data_ptr(), body.data_ptr(), rgb.data_ptr()))
            t1 = time.perf_counter()
            ctx.check(ctx.lib.atmrt_sky_shade_device(ctx.handle, C.byref(shade), bodies, n_bodies, true.data_ptr(), status.data_ptr(), column.data_ptr(),
                                                     body.data_ptr(), rgb.data_ptr()))
            t2 = time.perf_counter()
            if i >= a.warmup:
                t_bodies.append((t1 - t0) * 1e3), t_shade.append((t2 - t1) * 1e3), t_kernel.append(generators.sky_shade_timing(ctx))
        exits = status == _abi.SKY_EXIT
        x = (column / z0.value)[exits]
        out[f"step_{step:g}"] = dict(sky_march_ms=statistics.median(parent), light_march_ms=statistics.median(mine),
                                     bodies_call_ms=statistics.median(t_bodies), shade_call_ms=statistics.median(t_shade),
                                     shade_kernel_ms=statistics.median(t_kernel), zenith_column_m=z0.value, body_pixels=int((body != 0).sum()),
                                     air_mass_min=float(x.min()), air_mass_max=float(x.max()), **stats)
    print("RESULT " + json.dumps(out))
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--note", default=None, help="a line kept in the result, e.g. the build that ATMRT_LIB names")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    from atm_raytracer_amd import _lib
    runs = []
    for _ in range(a.processes):  # one after the other: a fresh process each, never two on the device at once
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(a.warmup), "--repeats", str(a.repeats),
                            "--width", str(a.width), "--height", str(a.height)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 1
        runs.append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
        print(f"process {len(runs)} of {a.processes}: light march {runs[-1]['step_1000']['light_march_ms']:.1f} ms, sky march "
              f"{runs[-1]['step_1000']['sky_march_ms']:.1f} ms at 1000 m", file=sys.stderr, flush=True)
    result = {"source_hash": _lib.source_hash(), "frame_px": [a.width, a.height], "top_m": TOP, "floor_m": FLOOR,
              "method": f"median over {a.processes} fresh processes of the median over {a.repeats} calls after {a.warmup} warm-up; march times between "
                        "events on the library's stream (atmrt_last_sky_timings), the two marches alternating in one process; shade and bodies "
                        "calls by the host's clock, the shade's kernel between events"}
    if a.note:
        result["note"] = a.note
    for key in runs[0]:
        v = result[key] = {k: statistics.median(r[key][k] for r in runs) for k in runs[0][key]}
        v["march_ratio"] = v["light_march_ms"] / v["sky_march_ms"]
        v["shade_call_ratio"] = v["shade_call_ms"] / v["bodies_call_ms"]
        v["light_steps_per_second"] = v["integrated_steps"] / (v["light_march_ms"] * 1e-3)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
