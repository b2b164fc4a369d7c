#!/usr/bin/env python3
"""Times atmrt_sky_directions_device on the headline frame (scene "headline": nine tiles, observer 500 m above the ground, refraction
on, step 100 m, 4096 x 2048, Rectilinear) to a top of 100 km with the sky step at 100 m and at 1000 m, in both list orders (the
march takes the compacted list from its end, where the horizon rows lie, or — ATMRT_SKY_ORDER=forward — from its head).  The library
reports where the time of a call went (atmrt_last_sky_timings: compaction, march, download between events on its stream) and what the
march did (the counts of atmrt_sky_stats_t); from those the march's integrated steps per second.  The figure to set beside it is the
cast-shadow march with its shortcut off (profiles/shadows.json, elevation_15_escape_off): one RK4 step per integrated step there
too, plus a geodesic point and a terrain sample that the sky march does not have.

Every figure is the median over --processes fresh processes of the median over --repeats calls after --warmup calls.

    python tools/measure_sky.py --out profiles/sky.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

TOP, FLOOR = 100_000.0, 0.0
STEPS = (100.0, 1000.0)


def child(a):
    import torch
    from atm_raytracer_amd import _abi, generators, synth
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", a.width, a.height, generator="Rectilinear")
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    dev = torch.device("cuda", 0)
    planes, pod = generators.image_planes(a.height, a.width, dev)
    gen.generate_device(pod)
    true = torch.empty((a.height, a.width), dtype=torch.float64, device=dev)
    status = torch.empty((a.height, a.width), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    out = {}

    def run(step):
        spec, st = generators.sky_spec(step, TOP, FLOOR), _abi.SkyStats()
        parts = {}
        for i in range(a.warmup + a.repeats):
            ctx.check(ctx.lib.atmrt_sky_directions_device(ctx.handle, C.byref(spec), true.data_ptr(), status.data_ptr(), None, C.byref(st)))
            if i >= a.warmup:
                for k, v in generators.sky_timings(ctx).items():
                    parts.setdefault(k, []).append(v)
        return dict({k: statistics.median(v) for k, v in parts.items()}, **generators._sky_stats(st))

    for order in ("reverse", "forward"):
        if order == "forward":
            os.environ["ATMRT_SKY_ORDER"] = "forward"
        for step in STEPS:
            out[f"step_{step:g}_{order}"] = run(step)
        os.environ.pop("ATMRT_SKY_ORDER", None)
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
        print(f"process {len(runs)} of {a.processes}: march {runs[-1]['step_100_reverse']['march_ms']:.1f} ms at 100 m", file=sys.stderr, flush=True)
    result = {"source_hash": _lib.source_hash(), "frame_px": [a.width, a.height], "top_m": TOP, "floor_m": FLOOR,
              "method": f"median over {a.processes} fresh processes of the median over {a.repeats} calls after {a.warmup} warm-up; times between "
                        "events on the library's stream (atmrt_last_sky_timings)"}
    for key in runs[0]:
        v = result[key] = {k: statistics.median(r[key][k] for r in runs) for k in runs[0][key]}
        v["integrated_steps_per_second"] = v["integrated_steps"] / (v["march_ms"] * 1e-3)
    try:
        with open(os.path.join(ROOT, "profiles", "shadows.json")) as fh:
            shadow = json.load(fh)["elevation_15_escape_off"]["integrated_steps_per_second"]
        result["shadow_march_escape_off_steps_per_second"] = shadow
        for key in runs[0]:
            result[key]["ratio_to_shadow_march_escape_off"] = result[key]["integrated_steps_per_second"] / shadow
    except (OSError, KeyError):
        pass
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
