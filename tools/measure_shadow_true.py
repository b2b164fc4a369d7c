#!/usr/bin/env python3
"""Times the true-direction shadow lights (include/atmrt.h, "apparent elevation") on the headline frame (scene "headline": nine
tiles, observer 500 m above the ground, refraction on, step 100 m, 4096 x 2048, Rectilinear) with a reach of 50 km:

  - the build of the refraction table for the default lattice (33 altitudes x 4601 launch elevations, sky step 1000 m, top 100 km):
    atmrt_last_sky_table_work's march, tail and download, each build under a key of its own (the step cap m alternates between two
    values that no ray reaches), and the same call when it finds the table;
  - atmrt_shadow_lights_device (the light's geometric direction: the call as it was before this rule) and
    atmrt_shadow_lights_true_device (the table found) for one light 5 degrees up and for a sunset light at the true elevation
    -0.3 degrees, both seen from the observer to the south-west: atmrt_last_shadow_timings and the counts of each call;
  - per light the share of hit pixels whose LIT bit differs between the two rules.

Every figure is the median over --processes fresh processes of the median over --repeats calls after --warmup calls; both rules
run in the same processes, one call after the other.

    python tools/measure_shadow_true.py --out profiles/shadow_true.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

REACH, AZIMUTH, SKY_STEP = 50_000.0, 225.0, 1000.0
LIGHTS = {"elevation_5": 5.0, "sunset_true_minus_0.3": -0.3}


def child(a):
    import torch
    from atm_raytracer_amd import _abi, generators, synth
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", a.width, a.height, generator="Rectilinear")
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    dev = torch.device("cuda", 0)
    planes, pod = generators.image_planes(a.height, a.width, dev)
    gen.generate_device(pod)
    masks = [torch.empty((a.height, a.width), dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize(dev)
    out = {}
    # the table: every build under another key, then the call that finds it
    builds, found = {}, {}
    table = generators.sky_table_spec(step=SKY_STEP)
    for i in range(a.warmup + a.repeats):
        spec = generators.sky_table_spec(step=SKY_STEP, m=generators.SKY_M - (i % 2))
        t = generators.sky_table(ctx, spec, planes=False)
        assert t.rebuilt == 1
        if i >= a.warmup:
            for k, v in t.ms.items():
                builds.setdefault(k, []).append(v)
    first = generators.sky_table(ctx, table, planes=False)
    for i in range(a.warmup + a.repeats):
        t = generators.sky_table(ctx, table, planes=False)
        assert t.rebuilt == 0
        if i >= a.warmup:
            for k, v in t.ms.items():
                found.setdefault(k, []).append(v)
    out["table"] = dict(n_alt=table.n_alt, n_el=table.n_el, sky_step_m=SKY_STEP, usable_rows=int(first.usable.sum()), tail_min=int(first.tail.min()),
                        tail_max=int(first.tail.max()), build={k: statistics.median(v) for k, v in builds.items()},
                        found={k: statistics.median(v) for k, v in found.items()}, **first.stats)

    def run(call, mask):
        st, parts = _abi.ShadowStats(), {}
        for i in range(a.warmup + a.repeats):
            call(mask, st)
            if i >= a.warmup:
                for k, v in generators.shadow_timings(ctx).items():
                    parts.setdefault(k, []).append(v)
        return dict({k: statistics.median(v) for k, v in parts.items()}, **generators._shadow_stats(st))

    for name, elevation in LIGHTS.items():
        lights, keep = generators.shadow_lights_spec(generators.lights_from_angles(cfg.params, [(AZIMUTH, elevation)], ctx.lib), REACH)
        geometric = run(lambda m, st: ctx.check(ctx.lib.atmrt_shadow_lights_device(ctx.handle, C.byref(lights), m.data_ptr(), None, None, C.byref(st))), masks[0])
        true = run(lambda m, st: ctx.check(ctx.lib.atmrt_shadow_lights_true_device(ctx.handle, C.byref(lights), C.byref(table), m.data_ptr(), None, None,
                                                                                  C.byref(st))), masks[1])
        assert generators.sky_table_work(ctx)[0] == 0
        hit = a.width * a.height - true["none"]
        differ = int((masks[0] != masks[1]).sum())
        out[name] = dict(azimuth_deg=AZIMUTH, elevation_deg=elevation, geometric=geometric, true=true, lit_bit_differs_px=differ,
                         lit_bit_differs_share_of_hit_px=differ / max(hit, 1))
    print("RESULT " + json.dumps(out))
    ctx.close()
    return 0


def median_tree(nodes):
    """The median, leaf by leaf, of equally shaped trees of numbers."""
    if isinstance(nodes[0], dict):
        return {k: median_tree([n[k] for n in nodes]) for k in nodes[0]}
    return statistics.median(nodes)


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
        print(f"process {len(runs)} of {a.processes}: table build {runs[-1]['table']['build']['march_ms']:.1f} ms, true march at 5 degrees "
              f"{runs[-1]['elevation_5']['true']['march_ms']:.1f} ms", file=sys.stderr, flush=True)
    result = {"source_hash": _lib.source_hash(), "frame_px": [a.width, a.height], "reach_m": REACH,
              "method": f"median over {a.processes} fresh processes of the median over {a.repeats} calls after {a.warmup} warm-up; times between "
                        "events on the library's stream (atmrt_last_sky_table_work, atmrt_last_shadow_timings); `geometric` is "
                        "atmrt_shadow_lights_device, the call as it was before the true-direction rule, in the same processes"}
    result.update(median_tree(runs))
    for name in LIGHTS:
        v = result[name]
        v["true_over_geometric_march"] = v["true"]["march_ms"] / v["geometric"]["march_ms"]
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
