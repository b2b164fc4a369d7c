"""The whole-frame work queue of the opaque Rectilinear march (k_rect_march_queue): a persistent kernel whose
wavefronts claim groups of 64 consecutive pixels from a queue sorted by estimated length and march each with the per-ray code of
the plain k_rect_march.  Only large frames take it by default, so the tests force it (ATMRT_MARCH_VARIANT=queue, read once per
process: child processes, as in test_gpu_march_variants.py) on scene S2 and require the bits and the counters of the plain kernel:
  * 160x96 (240 groups: 15 whole chunks of the 16 a short wavefront claims), twice in one context (the claim word is reset);
  * 150x61 with 26 m steps: a pixel count that is no multiple of 64 or 1024 (143 groups: no whole number of chunks), rays of many steps;
  * 200x37: 116 groups, the last one partial; 40x24: 15 groups, fewer than the wavefronts of ONE workgroup, so most claim nothing;
    64x1: a single group;
  * ATMRT_CEILING=rebuild (the order is built again in every frame) and two long wavefronts per SIMD instead of one: the same;
  * ATMRT_CEILING=off: no table, no order — the forced queue leaves the frames to the choice by size (here the time-sliced march);
    translucent terrain and objects never take it, nor does a column shard of the first frame (col_begin 64, col_end 160).
The order every queued frame marched with is read back (atmrt_debug_march_order) and must be a permutation of its groups, and
every frame says which route it was launched by (atmrt_debug_last_march_route; the plan: csrc/atmrt_march_plan.h)."""
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, hashlib, json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from atm_raytracer_amd import generators, synth
from util import run_gpu, FIELDS_PIXEL, FIELDS_HIT, bits, frame_stats
ctx = generators.Context(0)
out = {{}}
for name, kw, objects, size in (("opaque", dict(), False, (160, 96)), ("opaque-again", dict(), False, (160, 96)),
                                ("ragged", dict(step=26.0), False, (150, 61)), ("partial", dict(), False, (200, 37)),
                                ("tiny", dict(), False, (40, 24)), ("one", dict(), False, (64, 1)),
                                ("translucent", dict(terrain_alpha=0.5), False, (160, 96)), ("objects", dict(), True, (160, 96)),
                                ("shard", dict(), False, (160, 96))):
    cfg, tiles = synth.scene("S2", size[0], size[1], generator="Rectilinear", **{{**dict(max_distance=60_000.0, tilt=-1.0), **kw}})
    if name == "shard":  # `opaque` as a column shard: never the whole image, so never the queue
        cfg.params.col_begin, cfg.params.col_end = 64, 160
        size = (96, 96)
    if objects:
        synth.add_objects(cfg, n_cyl=40, n_bill=10, dist=(300.0, 20_000.0), spread_deg=30.0, radius=(30.0, 120.0), height=(150.0, 600.0),
                          bill_w=(150.0, 500.0), bill_h=(150.0, 500.0))
    r = run_gpu(ctx, cfg, tiles)
    h = hashlib.sha256()
    for k in FIELDS_PIXEL + FIELDS_HIT:
        h.update(np.ascontiguousarray(bits(r[k])).tobytes())
    integrated, escaped = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(integrated), C.byref(escaped)))
    order = ctx.debug_march_order()
    groups = (size[0] * size[1] + 63) // 64
    permutation = order.size == groups and bool((np.sort(order) == np.arange(groups, dtype=np.uint32)).all())
    out[name] = dict(frame=[h.hexdigest(), int(r["n_hits"]), int(r["ray_steps"]), int(frame_stats(ctx)["terrain_lookups"]),
                            int(integrated.value), int(escaped.value)],
                     queued=int(order.size), permutation=permutation, route=ctx.debug_march_route())
print("RESULT " + json.dumps(out))
"""
OPAQUE = ("opaque", "opaque-again", "ragged", "partial", "tiny", "one")
GROUPS = dict(zip(OPAQUE, (240, 240, 143, 116, 15, 1)))  # ceil(pixels / 64)


@functools.lru_cache(maxsize=None)
def _run(variant, **extra):
    env = dict(os.environ, ATMRT_MARCH_VARIANT=variant, **extra)
    for k in ("ATMRT_CEILING", "ATMRT_MARCH_QUEUE_LONG"):
        if k not in extra:
            env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _frames(run):
    """What must be equal between two runs: of the opaque frames the bits and every counter; of the translucent and the object scene,
    which never take the queue, the bits, the hits and the ray-steps — with the queue forced their launches go by their size (the
    small-launch march), whose work counters for an object scene are not the plain kernel's (it keeps the rays that one hands to the
    general tracer): the comparison test_gpu_march_variants.py makes."""
    return {name: r["frame"] if name in OPAQUE else r["frame"][:3] for name, r in run.items()}


@pytest.mark.gpu
def test_the_plain_frames_are_what_the_queue_is_compared_with():
    plain = _run("plain")
    assert all(r["queued"] == 0 for r in plain.values()), "the plain variant must not build an order"
    assert plain["opaque"]["frame"] == plain["opaque-again"]["frame"]
    assert plain["opaque"]["frame"][1] > 1000 and plain["ragged"]["frame"][1] > 500 and plain["tiny"]["frame"][1] > 0
    assert plain["opaque"]["frame"][5] > 0, "the scene must have rays that escape"
    assert plain["translucent"]["frame"][1] > plain["opaque"]["frame"][1] and plain["objects"]["frame"][1] > 0


@pytest.mark.gpu
def test_the_queue_gives_the_bits_and_counters_of_the_plain_march():
    plain, queue = _run("plain"), _run("queue")
    for name in OPAQUE:  # the opaque frames took the queue, over an order that is a permutation of their groups
        assert queue[name]["queued"] == GROUPS[name] and queue[name]["permutation"], (name, queue[name])
        assert queue[name]["route"] == 4, (name, queue[name])  # MarchRoute::Queue: launched, not only planned
    for name in ("translucent", "objects"):  # these never do: the small-launch grid, by their size
        assert queue[name]["queued"] == 0 and queue[name]["route"] == 2, (name, queue[name])
    # a column shard is not the whole image: no order is built for it and it stays on the time-sliced march
    assert queue["shard"]["queued"] == 0 and queue["shard"]["route"] == 3, queue["shard"]
    assert queue["shard"]["frame"][:3] == plain["shard"]["frame"][:3] and plain["shard"]["route"] == 1
    assert _frames(queue) == _frames(plain)
    assert queue["opaque"]["frame"] == queue["opaque-again"]["frame"], "the second frame of a context starts from a fresh claim word"


@pytest.mark.gpu
def test_an_order_rebuilt_in_every_frame_and_two_long_wavefronts_per_simd_change_nothing():
    plain = _run("plain")
    rebuilt = _run("queue", ATMRT_CEILING="rebuild")
    assert all(rebuilt[name]["queued"] == GROUPS[name] and rebuilt[name]["permutation"] for name in OPAQUE)
    assert _frames(rebuilt) == _frames(plain)
    two = _run("queue", ATMRT_MARCH_QUEUE_LONG="2")
    assert all(two[name]["queued"] == GROUPS[name] for name in OPAQUE)
    assert _frames(two) == _frames(plain)


@pytest.mark.gpu
def test_without_a_ceiling_table_the_forced_queue_falls_back_to_the_grid():
    off = _run("queue", ATMRT_CEILING="off")
    assert all(r["queued"] == 0 for r in off.values())
    assert all(off[name]["route"] == 3 for name in OPAQUE), "small opaque launches without an order: the time-sliced march, not the queue"
    # without the table fewer samples skip their lookup and rays leave later: the work counters differ from the table's; the image,
    # its hits and the ray-steps (credited steps included) do not
    assert {k: f[:3] for k, f in _frames(off).items()} == {k: f[:3] for k, f in _frames(_run("plain")).items()}
