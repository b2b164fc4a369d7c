#!/usr/bin/env python3
"""Times atmrt_shadow_mask_device on the headline frame (scene "headline": nine tiles, observer 500 m above the ground, refraction
on, step 100 m, 4096 x 2048, Rectilinear) for lights 5, 15 and 45 degrees high at azimuth 225, reach 50 km (m = 500), lift 0, and at
15 degrees with the escape shortcut off (ATMRT_SHADOW_ESCAPE=off).  The library reports where the time of a call went
(atmrt_last_shadow_timings: compaction, march, download between events on its stream) and what the march did (integrated_steps,
escaped_rays); from those the march's integrated ray-steps per second.  Beside it the same figure of the frame's own march,
k_rect_march, on the same frame in the same process: atmrt_last_march_work's integrated steps over atmrt_last_timings' march_ms.
Both kernels take one RK4 step and at most one terrain sample per integrated step.

Every figure is the median over --processes fresh processes of the median over --repeats calls after --warmup calls.

    python tools/measure_shadows.py --out profiles/shadows.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ELEVATIONS = (5.0, 15.0, 45.0)
AZIMUTH, REACH = 225.0, 50_000.0


def child(a):
    import torch
    from atm_raytracer_amd import _abi, generators, synth
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", a.width, a.height, generator="Rectilinear")
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    dev = torch.device("cuda", 0)
    planes, pod = generators.image_planes(a.height, a.width, dev)
    frame_ms, frame_steps = [], 0
    for i in range(a.warmup + a.repeats):
        gen.generate_device(pod)
        if i >= a.warmup:
            steps, esc = C.c_uint64(), C.c_uint64()
            ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(steps), C.byref(esc)))
            frame_ms.append(gen.last_timings()["march_ms"])
            frame_steps = steps.value
    out = {"frame": {"march_ms": statistics.median(frame_ms), "integrated_steps": frame_steps,
                     "hit_pixels": int((planes["hit_count"] > 0).sum().item())}}
    status = torch.empty((a.height, a.width), dtype=torch.uint8, device=dev)

    def run(elevation):
        spec, st = generators.shadow_spec(AZIMUTH, elevation, REACH, 0.0), _abi.ShadowStats()
        parts = {}
        for i in range(a.warmup + a.repeats):
            ctx.check(ctx.lib.atmrt_shadow_mask_device(ctx.handle, C.byref(spec), status.data_ptr(), None, C.byref(st)))
            if i >= a.warmup:
                for k, v in generators.shadow_timings(ctx).items():
                    parts.setdefault(k, []).append(v)
        return dict({k: statistics.median(v) for k, v in parts.items()}, **generators._shadow_stats(st))

    for e in ELEVATIONS:
        out[f"elevation_{e:g}"] = run(e)
    os.environ["ATMRT_SHADOW_ESCAPE"] = "off"
    out["elevation_15_escape_off"] = run(15.0)
    del os.environ["ATMRT_SHADOW_ESCAPE"]
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
        print(f"process {len(runs)} of {a.processes}: frame march {runs[-1]['frame']['march_ms']:.1f} ms", file=sys.stderr, flush=True)
    result = {"source_hash": _lib.source_hash(), "frame_px": [a.width, a.height], "simulation_step_m": 100.0, "light_azimuth_deg": AZIMUTH,
              "reach_m": REACH, "lift_m": 0.0,
              "method": f"median over {a.processes} fresh processes of the median over {a.repeats} calls after {a.warmup} warm-up; times between "
                        "events on the library's stream (atmrt_last_shadow_timings, atmrt_last_timings)"}
    for key in runs[0]:
        result[key] = {k: statistics.median(r[key][k] for r in runs) for k in runs[0][key]}
    f = result["frame"]
    f["integrated_steps_per_second"] = f["integrated_steps"] / (f["march_ms"] * 1e-3)
    for key, v in result.items():
        if key.startswith("elevation_"):
            v["integrated_steps_per_second"] = v["integrated_steps"] / (v["march_ms"] * 1e-3)
            v["ratio_to_frame_march"] = v["integrated_steps_per_second"] / f["integrated_steps_per_second"]
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
