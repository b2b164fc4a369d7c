#!/usr/bin/env python3
"""Experiment: the wavefront timeline of a k_rect_march launch (library built with -DATMRT_TIMELINE, selected through ATMRT_LIB).

Shard mode — ONE column shard: per millisecond, how many wavefronts are resident and how many SIMDs hold at least 1 / 4 of them;
and the long wavefronts that end last.
    ATMRT_LIB=.../dev/tl/libatmrt.so python tools/measure_march_timeline.py [G [g]]
Whole-frame mode — the headline frame in one launch (plain k_rect_march: an entry per wavefront; k_rect_march_queue: an entry per
64-pixel group, written by the wavefront that marched it): per SIMD the wave-steps it was given and when its last wavefront ended,
the distribution of those sums, the longest single wavefront, and which SIMD the wavefronts of a workgroup run on.
    ATMRT_LIB=.../dev/tl/libatmrt.so python tools/measure_march_timeline.py whole [OUT.txt]"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from atm_raytracer_amd import _lib, generators, synth  # noqa: E402

W, H = 4096, 2048
WHOLE = len(sys.argv) > 1 and sys.argv[1] == "whole"
G = 1 if WHOLE else int(sys.argv[1]) if len(sys.argv) > 1 else 8
g = 0 if WHOLE else int(sys.argv[2]) if len(sys.argv) > 2 else 3
TIMELINE_WAVES = 262144  # atmrt_march_impl.h
cfg, tiles = synth.scene("headline", W, H, generator="Rectilinear", level=2)
ctx = generators.Context(0)
terrain = generators.Terrain.from_tiles(tiles, ctx)
c0, c1 = g * W // G, (g + 1) * W // G
if not WHOLE:
    cfg.params.col_begin, cfg.params.col_end = c0, c1
_planes, slab_pod = generators.image_planes(H, c1 - c0, torch.device("cuda", 0))
gen = generators.make_generator(generators.Params(cfg), terrain)
for _ in range(4):
    steps, ms = gen.generate_device(slab_pod)
n_waves = (c1 - c0) * H // 64
assert n_waves <= TIMELINE_WAVES
buf = np.zeros(3 * n_waves, dtype=np.uint64)
lib = _lib.load()
lib.atmrt_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
rc = lib.atmrt_debug_timeline(buf.ctypes.data, buf.size)
assert rc == 0, rc
t = buf.reshape(-1, 3)[:n_waves]
t0 = t[:, 0].astype(np.int64)
t1 = t[:, 1].astype(np.int64)
base = t0.min()
st = (t0 - base) / 100e3  # 100 MHz -> ms
en = (t1 - base) / 100e3
wsteps = (t[:, 2] & np.uint64(0xfffff)).astype(np.int64)  # ray-steps of the 64 lanes, credited escape steps included
wg_wave = ((t[:, 2] >> np.uint64(20)) & np.uint64(0xf)).astype(np.int64)
hw = ((t[:, 2] >> np.uint64(24)) & np.uint64(0xffff)).astype(np.int64)
xcc = ((t[:, 2] >> np.uint64(40)) & np.uint64(0xf)).astype(np.int64)
loop = ((t[:, 2] >> np.uint64(44)) & np.uint64(0xfffff)).astype(np.int64)  # wave-steps: iterations of the wavefront's step loop
simd = (hw >> 4) & 3
cu = (hw >> 8) & 15
se = (hw >> 13) & 7
cu_key = (xcc * 8 + se) * 16 + cu
simd_key = cu_key * 4 + simd
wl = c1 - c0
# the queue's view of every group: its position in the order, and (a library with atmrt_debug_timeline_estimates) the estimate it
# was sorted by and whether a long wavefront marched it
position = estimate = by_long = None
if WHOLE:
    order = ctx.debug_march_order()
    if order.size == n_waves:
        position = np.empty(n_waves, dtype=np.int64)
        position[order] = np.arange(n_waves)
        if hasattr(lib, "atmrt_debug_timeline_estimates"):
            est = np.zeros(n_waves, dtype=np.uint32)
            lib.atmrt_debug_timeline_estimates.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
            assert lib.atmrt_debug_timeline_estimates(est.ctypes.data, est.size) == 0
            estimate = (est & np.uint32(0x7fffffff)).astype(np.int64)
            by_long = (est >> np.uint32(31)).astype(np.int64)


def whole_frame(out):
    def p(*a):
        print(*a, file=out)
    span = float(en.max())
    dur = en - st
    keys, inv = np.unique(simd_key, return_inverse=True)
    work = np.bincount(inv, weights=loop).astype(np.int64)
    count = np.bincount(inv)
    last = np.zeros(len(keys))
    np.maximum.at(last, inv, en)
    p(f"whole frame {W}x{H}: {n_waves} entries, march event time {ms:.3f} ms, timeline span {span:.3f} ms, distinct SIMDs {len(keys)}")
    p(f"wave-steps in all {int(loop.sum())}; per SIMD mean {work.mean():.0f} p50 {np.quantile(work, 0.5):.0f} p99 {np.quantile(work, 0.99):.0f} "
      f"max {work.max()} min {work.min()}")
    p(f"end of the last wavefront per SIMD (ms): mean {last.mean():.3f} p50 {np.quantile(last, 0.5):.3f} p99 {np.quantile(last, 0.99):.3f} "
      f"max {last.max():.3f} min {last.min():.3f}")
    k = int(np.argmax(dur))
    p(f"longest single entry: {dur[k]:.3f} ms = {dur[k] / span:.3f} of the span ({loop[k]} wave-steps, group {k}, row {k * 64 // wl}, "
      f"start {st[k]:.3f} ms); per wave-step {1e3 * dur[k] / max(loop[k], 1):.2f} us")
    def queue_columns(w):  # position in the order, estimate, L = marched by a long wavefront
        if position is None:
            return ""
        return f" pos {position[w]:6d}" + ("" if estimate is None else f" est {estimate[w]:5d} {'L' if by_long[w] else 's'}")
    p(f"span minus the mean end of a SIMD: {span - last.mean():.3f} ms; the launch ends with group {int(np.argmax(en))}, "
      f"started at {st[int(np.argmax(en))]:.3f} ms")
    if estimate is not None:
        p(f"estimate of the head {estimate[position == 0][0]}; entries marched by long wavefronts {int(by_long.sum())}")
        head = int(estimate[position == 0][0])
        eighth = (head + 7) // 8
        p(f"entries that outrun their estimate: by an eighth of the head's ({eighth}) {int((loop > estimate + eighth).sum())}, by a quarter "
          f"{int((loop > estimate + 2 * eighth).sum())}; to twice the estimate and past a quarter of the head's "
          f"{int(((loop >= 2 * estimate) & (loop >= 2 * eighth)).sum())}")
        p("largest wave-steps minus estimate: (group, row, start, end, wave-steps, us per wave-step, position in the order, estimate, long / short)")
        for w in np.argsort(-(loop - estimate))[:12]:
            p(f"  {w:6d} row {w * 64 // wl:5d} {st[w]:7.3f} {en[w]:7.3f} {loop[w]:6d} {1e3 * dur[w] / max(loop[w], 1):6.2f}{queue_columns(w)}")
    p("most wave-steps: (group, row, start, end, wave-steps, us per wave-step[, position in the order, estimate, long / short])")
    for w in np.argsort(-loop)[:10]:
        p(f"  {w:6d} row {w * 64 // wl:5d} {st[w]:7.3f} {en[w]:7.3f} {loop[w]:6d} {1e3 * dur[w] / max(loop[w], 1):6.2f}{queue_columns(w)}")
    p("last to end: (group, row, start, end, wave-steps, SIMD key[, position in the order, estimate, long / short])")
    for w in np.argsort(-en)[:10]:
        p(f"  {w:6d} row {w * 64 // wl:5d} {st[w]:7.3f} {en[w]:7.3f} {loop[w]:6d} {simd_key[w]:6d}{queue_columns(w)}")
    heavy = loop >= 250
    p(f"entries of >= 250 wave-steps: {int(heavy.sum())}, carrying {int(loop[heavy].sum())} wave-steps; per SIMD mean "
      f"{np.bincount(inv, weights=heavy).mean():.2f} max {int(np.bincount(inv, weights=heavy).max())}")
    # which SIMD the wavefronts of a workgroup run on: per CU, the SIMDs seen for every wavefront index of the workgroup
    n_wg_waves = int(wg_wave.max()) + 1
    if n_wg_waves <= 4:  # the plain grid: entry w is wavefront w % 4 of workgroup w / 4
        full = n_waves // 4 * 4
        s4 = simd[:full].reshape(-1, 4)
        distinct = np.array([len(set(r)) for r in s4[:: max(1, len(s4) // 4096)]])
        same_cu = (cu_key[:full].reshape(-1, 4) == cu_key[:full].reshape(-1, 4)[:, :1]).all()
        p(f"workgroups of 4 wavefronts: all on one CU {bool(same_cu)}; distinct SIMDs per workgroup (sample of {len(distinct)}): "
          f"{dict(zip(*[x.tolist() for x in np.unique(distinct, return_counts=True)]))}; "
          f"SIMD == wavefront index in {float((s4 == np.arange(4)).mean()):.3f} of the wavefronts")
    else:  # the queue: one workgroup per CU, entries written by wavefront wg_wave of the CU's workgroup
        table = np.full((int(cu_key.max()) + 1, 16), -1, dtype=np.int64)
        clash = 0
        for c, w_, s_ in zip(cu_key, wg_wave, simd):
            if table[c, w_] >= 0 and table[c, w_] != s_:
                clash += 1
            table[c, w_] = s_
        seen = table >= 0
        share = [(table[:, w_] == table[:, w_ % 4])[seen[:, w_] & seen[:, w_ % 4]].mean() for w_ in range(4, n_wg_waves)]
        p(f"workgroups of {n_wg_waves} wavefronts: a wavefront changed SIMD {clash} times; wavefront w shares the SIMD of w % 4 in "
          f"{np.mean(share):.3f} of the cases; SIMD == w % 4 in {float((table == np.arange(16) % 4)[seen].mean()):.3f}")
    p("per ms: entries running, SIMDs with >= 1 / >= 4 running")
    for a in np.arange(0.0, span + 0.5, 0.5):
        mid = a + 0.25
        on = (st <= mid) & (en > mid)
        _, counts = np.unique(simd_key[on], return_counts=True)
        p(f"{mid:6.2f} {int(on.sum()):7d} {len(counts):6d} {int((counts >= 4).sum()):6d}")
    p("per SIMD: key (((xcc * 8 + se) * 16 + cu) * 4 + simd), entries, wave-steps, end of its last wavefront in ms")
    for q in np.argsort(-last):
        p(f"{keys[q]:6d} {count[q]:6d} {work[q]:8d} {last[q]:8.3f}")
    return {"event_ms": ms, "span_ms": span, "simd_end_mean_ms": float(last.mean()), "span_minus_simd_end_ms": float(span - last.mean()),
            "last_group": int(np.argmax(en)), "last_group_start_ms": float(st[int(np.argmax(en))]), "longest_ms": float(dur[k]), "longest_frac": float(dur[k] / span),
            "wave_steps": int(loop.sum()), "simd_work_mean": float(work.mean()), "simd_work_max": int(work.max())}


if WHOLE:
    path = sys.argv[2] if len(sys.argv) > 2 else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with (open(path, "w") if path else sys.stdout) as fh:
        summary = whole_frame(fh)
    print(json.dumps(summary))
    sys.exit(0)

print(f"shard {g} of {G}: {n_waves} wavefronts, event time {ms:.2f} ms, span {en.max():.2f} ms, distinct SIMDs {len(np.unique(simd_key))}")
long_ = wsteps >= 64 * 1900
print(f"long wavefronts (>= 1900 steps on every lane): {long_.sum()}; work in wave-steps: long {wsteps[long_].sum():.3g} of {wsteps.sum():.3g}")
edges = np.arange(0.0, en.max() + 1.0, 1.0)
print(" ms  resident  long  SIMDs>=1  SIMDs>=4  SIMDs>=5")
for a in edges:
    mid = a + 0.5
    on = (st <= mid) & (en > mid)
    keys, counts = np.unique(simd_key[on], return_counts=True)
    print(f"{mid:5.1f} {on.sum():7d} {int((on & long_).sum()):6d} {len(keys):8d} {int((counts >= 4).sum()):8d} {int((counts >= 5).sum()):8d}")
order = np.argsort(-en)[:12]
print("last to end: (wave, row, start, end, duration, steps/lane)")
for w in order:
    print(f"  {w:6d} row {w * 64 // wl:5d}  {st[w]:7.2f} {en[w]:7.2f} {en[w] - st[w]:7.2f} {wsteps[w] / 64:8.1f}")
dur = en - st
print("duration of long wavefronts by start time: quantiles of start", np.quantile(st[long_], [0, 0.5, 0.9, 0.99, 1]).round(2),
      "duration", np.quantile(dur[long_], [0, 0.1, 0.5, 0.9, 1]).round(2))
late = long_ & (st > 1.0)
if late.any():
    print(f"long wavefronts that started after 1 ms: {late.sum()}, start {st[late].min():.2f}..{st[late].max():.2f}, duration "
          f"{dur[late].min():.2f}..{dur[late].max():.2f}, end {en[late].min():.2f}..{en[late].max():.2f}")
print(json.dumps({"G": G, "g": g, "event_ms": ms, "span_ms": float(en.max()), "waves": int(n_waves), "long": int(long_.sum())}))
