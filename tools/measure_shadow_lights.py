#!/usr/bin/env python3
"""Times atmrt_shadow_lights_device on the headline frame of tools/measure_shadows.py (scene "headline": nine tiles, observer 500 m
above the ground, refraction on, step 100 m, 4096 x 2048, Rectilinear; reach 50 km, m = 500, lift 0) for four settings: one light 5,
15 and 45 degrees high at azimuth 225 as seen from the observer, and 24 lights along an arc from (azimuth 90, elevation 2) to
(azimuth 225, elevation 45).  A call writes the lit mask alone.  Per setting: compaction and march in milliseconds between events
on the library's stream (atmrt_last_shadow_timings) and the march's integrated ray-steps per second.

Beside each, the only route the parent commit has, timed in the same process: that many calls of atmrt_shadow_mask_device at the
same angles as seen from the observer (the fixed-direction rule: not the same answer, the same kind of work), their compaction and
march times and their integrated steps summed.

Every figure is the median over --processes fresh processes of the median over --repeats calls after --warmup calls.

    python tools/measure_shadow_lights.py --out profiles/shadow_lights.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

AZIMUTH, REACH = 225.0, 50_000.0
SETTINGS = {"one_light_5": [(AZIMUTH, 5.0)], "one_light_15": [(AZIMUTH, 15.0)], "one_light_45": [(AZIMUTH, 45.0)],
            "arc_24_lights": [(90.0 + 135.0 * k / 23.0, 2.0 + 43.0 * k / 23.0) for k in range(24)]}


def child(a):
    import torch
    from atm_raytracer_amd import _abi, generators, synth
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", a.width, a.height, generator="Rectilinear")
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    dev = torch.device("cuda", 0)
    planes, pod = generators.image_planes(a.height, a.width, dev)
    gen.generate_device(pod)
    mask = torch.empty((a.height, a.width), dtype=torch.int64, device=dev)
    status = torch.empty((a.height, a.width), dtype=torch.uint8, device=dev)
    out = {"hit_pixels": int((planes["hit_count"] > 0).sum().item())}

    def timed(call):
        """call() -> stats dict; the medians of the call's parts over the repeats, and the last call's counts."""
        parts, stats = {}, None
        for i in range(a.warmup + a.repeats):
            stats, t = call()
            if i >= a.warmup:
                for k, v in t.items():
                    parts.setdefault(k, []).append(v)
        return dict({k: statistics.median(v) for k, v in parts.items()}, **stats)

    for name, rows in SETTINGS.items():
        spec, keep = generators.shadow_lights_spec(generators.lights_from_angles(cfg.params, rows, ctx.lib), REACH, 0.0)

        def lights_call():
            st = _abi.ShadowStats()
            ctx.check(ctx.lib.atmrt_shadow_lights_device(ctx.handle, C.byref(spec), mask.data_ptr(), None, None, C.byref(st)))
            return generators._shadow_stats(st), generators.shadow_timings(ctx)

        def single_calls():
            total, t = {}, {}
            for az, el in rows:
                one, st = generators.shadow_spec(az, el, REACH, 0.0), _abi.ShadowStats()
                ctx.check(ctx.lib.atmrt_shadow_mask_device(ctx.handle, C.byref(one), status.data_ptr(), None, C.byref(st)))
                for k, v in generators._shadow_stats(st).items():
                    total[k] = total.get(k, 0) + v
                for k, v in generators.shadow_timings(ctx).items():
                    t[k] = t.get(k, 0.0) + v
            return total, t

        out[name] = {"n_lights": len(rows), "lights_call": timed(lights_call), "single_calls": timed(single_calls)}
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
        print(f"process {len(runs)} of {a.processes}: 24 lights march {runs[-1]['arc_24_lights']['lights_call']['march_ms']:.1f} ms", file=sys.stderr, flush=True)
    result = {"source_hash": _lib.source_hash(), "frame_px": [a.width, a.height], "simulation_step_m": 100.0, "reach_m": REACH, "lift_m": 0.0,
              "hit_pixels": runs[0]["hit_pixels"], "lights_deg": {k: v for k, v in SETTINGS.items()},
              "method": f"median over {a.processes} fresh processes of the median over {a.repeats} calls after {a.warmup} warm-up; times between "
                        "events on the library's stream (atmrt_last_shadow_timings); single_calls: n_lights calls of atmrt_shadow_mask_device "
                        "at the same angles as seen from the observer, times and steps summed"}
    for key in SETTINGS:
        entry = {"n_lights": runs[0][key]["n_lights"]}
        for route in ("lights_call", "single_calls"):
            v = {k: statistics.median(r[key][route][k] for r in runs) for k in runs[0][key][route]}
            v["integrated_steps_per_second"] = v["integrated_steps"] / (v["march_ms"] * 1e-3)
            entry[route] = v
        entry["lights_call_over_single_calls_ms"] = (entry["lights_call"]["compact_ms"] + entry["lights_call"]["march_ms"]) / \
            (entry["single_calls"]["compact_ms"] + entry["single_calls"]["march_ms"])
        result[key] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
