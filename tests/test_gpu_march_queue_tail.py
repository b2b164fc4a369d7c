"""The tail of the whole-frame work queue (k_rect_march_queue): what a long wavefront's priority goes by
(ATMRT_MARCH_QUEUE_PRIO) and how chunks shrink as the queue empties (ATMRT_MARCH_QUEUE_CHUNKS) decide scheduling only.  As in
test_gpu_march_queue.py the queue is forced (ATMRT_MARCH_VARIANT=queue, read once per process: child processes) on scene S2, under
every value of each switch and under their combinations, and every frame must have the bits and the counters of the plain kernel
— the digest of every plane, n_hits, ray_steps, terrain_lookups, integrated and escaped steps — over an order that is a
permutation of its groups.  Shapes, each the smallest of its kind:
  * 160x96: 240 groups, fewer than the wavefronts of the launch, so chunks are capped by what is left from the first claim on;
  * 150x61 with 26 m steps: 143 groups, rays of many steps, sky rows to skyline rows, so that the estimates of the order differ
    widely (which priorities a frame's estimates reach is not read back here and bit-identity cannot see it: the rule itself,
    queue_item_priority, is checked over its whole domain on the host, tests/csrc/claim_guided_host.cpp);
  * 40x24: 15 groups, fewer than the wavefronts of ONE workgroup, so most claim nothing; 64x1: one group, the head is its own
    reference estimate;
  * 160x96 a second time in the same context: the claim word starts from zero again."""
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
for name, kw, size in (("capped", dict(), (160, 96)), ("long", dict(step=26.0), (150, 61)), ("tiny", dict(), (40, 24)),
                       ("one", dict(), (64, 1)), ("capped-again", dict(), (160, 96))):
    cfg, tiles = synth.scene("S2", size[0], size[1], generator="Rectilinear", **{{**dict(max_distance=60_000.0, tilt=-1.0), **kw}})
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
                     queued=int(order.size), permutation=permutation)
print("RESULT " + json.dumps(out))
"""
GROUPS = dict(zip(("capped", "long", "tiny", "one", "capped-again"), (240, 143, 15, 1, 240)))  # ceil(pixels / 64)
SWITCHES = ("ATMRT_MARCH_QUEUE_PRIO", "ATMRT_MARCH_QUEUE_CHUNKS")
PRIO = ("role", "item")
CHUNKS = ("steps", "guided")


@functools.lru_cache(maxsize=None)
def _run(variant, **extra):
    env = dict(os.environ, ATMRT_MARCH_VARIANT=variant, **extra)
    for k in ("ATMRT_CEILING", "ATMRT_MARCH_QUEUE_LONG") + SWITCHES:
        if k not in extra:
            env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _same_as_plain(run):
    plain = _run("plain")
    for name, groups in GROUPS.items():
        assert run[name]["queued"] == groups and run[name]["permutation"], (name, run[name])
        assert run[name]["frame"] == plain[name]["frame"], name
    assert run["capped"]["frame"] == run["capped-again"]["frame"], "the second frame of a context starts from a fresh claim word"


@pytest.mark.gpu
def test_the_plain_frames_have_hits_escapes_and_long_rays():
    plain = _run("plain")
    assert all(r["queued"] == 0 for r in plain.values()), "the plain variant must not build an order"
    assert plain["capped"]["frame"][1] > 1000 and plain["long"]["frame"][1] > 500 and plain["tiny"]["frame"][1] > 0
    assert plain["capped"]["frame"][5] > 0, "the scene must have rays that escape"
    assert plain["long"]["frame"][4] > plain["capped"]["frame"][4] // 2, "the 26 m frame must integrate many steps per ray"


@pytest.mark.gpu
def test_the_defaults_give_the_bits_and_counters_of_the_plain_march():
    _same_as_plain(_run("queue"))


@pytest.mark.gpu
@pytest.mark.parametrize("prio", PRIO)
def test_every_priority_rule_changes_nothing(prio):
    _same_as_plain(_run("queue", ATMRT_MARCH_QUEUE_PRIO=prio))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", CHUNKS)
def test_either_chunk_rule_changes_nothing(chunks):
    _same_as_plain(_run("queue", ATMRT_MARCH_QUEUE_CHUNKS=chunks))


@pytest.mark.gpu
@pytest.mark.parametrize("prio,chunks", [(p, c) for p in PRIO for c in CHUNKS])
def test_the_switches_combined_change_nothing(prio, chunks):
    _same_as_plain(_run("queue", ATMRT_MARCH_QUEUE_PRIO=prio, ATMRT_MARCH_QUEUE_CHUNKS=chunks))


@pytest.mark.gpu
@pytest.mark.parametrize("n_long", ("1", "2", "3"))
def test_any_number_of_long_wavefronts_per_simd_under_the_new_rules_changes_nothing(n_long):
    _same_as_plain(_run("queue", ATMRT_MARCH_QUEUE_LONG=n_long))
