#!/usr/bin/env python3
"""Times atmrt_sight_lines at the headline's setting (scene "headline": nine tiles, observer 500 m above the ground, refraction on,
step 100 m) for 1, 64 and 1024 targets 200 km away (2000 samples each), fan -5 .. 5 degrees, 3 rounds.  Targets are spread evenly
over the azimuths, height 0.  The library reports where the time of a call went (atmrt_last_sight_timings: profile pass, solve and
download between events on its stream); the whole synchronous call is timed on the host clock besides.  No frame is generated:
the solve needs none, and the parent of the change that added it has no counterpart to compare with.

    python tools/measure_sight_lines.py --out profiles/sight_lines.json"""
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--distance", type=float, default=200_000.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ctx = generators.Context(0)
    cfg, tiles = synth.scene("headline", generator="Fast")
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))._configure()
    result = {"source_hash": _lib.source_hash(), "distance_m": a.distance, "simulation_step_m": cfg.params.simulation_step, "fan_deg": [-5.0, 5.0],
              "rounds": a.rounds,
              "method": "per call: atmrt_last_sight_timings (profile pass with its upload, solve, download between events on the library's "
                        "stream, summed over the call's batches) and the host clock around the whole synchronous call; median of repeats after warm-up",
              "parent_commit": "no counterpart: the library could not solve a sight line before this change",
              "cases": {}}
    for n in (int(x) for x in a.counts.split(",")):
        targets = np.zeros(n, dtype=generators.SIGHT_TARGET_DTYPE)
        targets["azimuth_deg"], targets["distance"] = np.arange(n) * (360.0 / n), a.distance
        parts, calls = {}, []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            got = generators.sight_lines(ctx, targets, (-5.0, 5.0), a.rounds)
            calls.append((time.perf_counter() - t0) * 1e3)
            if i >= a.warmup:
                for k, v in generators.sight_timings(ctx).items():
                    parts.setdefault(k, []).append(v)
        batches = parts.pop("batches")[0]
        result["cases"][f"targets_{n}"] = {
            "call_host_clock": spread(calls[a.warmup:]), **{k: spread(v) for k, v in parts.items()}, "batches": batches,
            "samples_per_target": int(got["m"].max()), "status_counts_seen_hidden_above_below": np.bincount(got["status"], minlength=4).tolist(),
            "rounds_done_counts": np.bincount(got["rounds_done"], minlength=a.rounds + 1).tolist()[1:]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
