"""atmrt_viewshed_map* on the GPU.  The expected map is always tests/viewshed_map_model.py (the rule of include/atmrt.h in numpy) applied
to the planes generators.viewshed returns on the same context — planes tests/test_gpu_viewshed.py pins bit for bit against the oracle —
never the output of the code under test.  Counts equal, min_hidden byte for byte, stats equal.  One synthetic level-1 tile, step 100 m.
Every case prints its figures before it asserts (`viewshed map <case>: ...`)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

import polar_plan_model as pm
import viewshed_map_model as mm
import viewshed_model as vm
from atm_raytracer_amd import _abi, generators, synth
from atmospheres import inversion

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 100.0
FAN = (-6.0, 6.0)
_TILES = {}


def scene(**over):
    """Scene S2 (one tile, observer 46.5 N 8.5 E, 50 m above the ground, refraction on, step 100 m) with 60 km of range."""
    over.setdefault("max_distance", 60_000.0)
    cfg, tiles = synth.scene("S2", 64, 48, generator="Fast", **over)
    if not _TILES:
        _TILES.update(tiles)
    return cfg, _TILES


def duct():
    cfg, tiles = scene(atmosphere=inversion(vm.DUCT["at"], vm.DUCT["thick"], vm.DUCT["gradient"]))
    cfg.params.position.altitude_kind, cfg.params.position.altitude = _abi.ALT_ABSOLUTE, vm.DUCT["altitude"]
    return cfg, tiles


SETTINGS = {"us76": (lambda: scene(), FAN), "duct": (duct, vm.DUCT["fan"])}  # the two of tests/test_gpu_viewshed.py's table the issue names


def configure(ctx, cfg, tiles):
    """The scene's terrain, parameters and atmosphere on the context, without a frame."""
    ctx.check(ctx.lib.atmrt_terrain_clear(ctx.handle))
    gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
    gen._configure()
    return gen


def shape():
    s = generators.viewshed_kernel_shape(64)
    two = next(K for K in range(64, 4097, 64) if generators.viewshed_kernel_shape(K)["rays_per_lane"] >= 2)
    return s["az_per_load"], s["step_tile"], two


def device(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def to_host(m):
    """A ViewshedMap of either route -> (n_samples, n_seen, min_hidden as numpy arrays, stats)."""
    def host(a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return host(m.n_samples).view(np.uint32), host(m.n_seen).view(np.uint32), host(m.min_hidden), m.stats


def expected(ctx, grid, call, into=None):
    """The model over the planes of generators.viewshed for the same call on the same context."""
    v = generators.viewshed(ctx, *call)
    return v, mm.bin_planes(grid, v.status, v.hidden, v.lat, v.lon, into)


def fused(ctx, grid, call, **kw):
    return generators.viewshed_map(ctx, grid, *call, into=generators.viewshed_map_tensors(grid, device(ctx)), **kw)


def same_bytes(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def observer_grid(cfg, reach, cell_deg):
    pos = cfg.params.position
    return generators.viewshed_map_grid(pos.latitude, pos.longitude, reach, cell_deg)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_scatter_shapes_equal_the_model(gpu_ctx, name):
    """One sample per lane, 256-thread blocks, 64-lane wavefronts: n_az * m of 1, 63, 64, 65, 255, 256, 257 at n_az = 1; the scan's
    own shape straddled, n_az in {A - 1, A, A + 1} x m in {tile - 1, tile, tile + 1}; K = 64 and the smallest K with two rays per lane."""
    make, fan = SETTINGS[name]
    cfg, tiles = make()
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    assert two > 64
    grid = observer_grid(cfg, 26_000.0, 30.0 / 3600.0)
    shapes = [(1, m) for m in (1, 63, 64, 65, 255, 256, 257)] + [(n_az, m) for n_az in (A - 1, A, A + 1) for m in (tile - 1, tile, tile + 1)]
    binned = seen = 0
    for n, (n_az, m) in enumerate(shapes):
        for K in (64, two):
            reach = 50.0 if m == 1 else m * STEP - 30.0
            call = (20.0, 17.5, n_az, reach, (0.0, 25.0)[n % 2], fan, K)
            v, want = expected(gpu_ctx, grid, call)
            got = to_host(fused(gpu_ctx, grid, call))
            print(f"viewshed map {name} n_az={n_az} m={m} K={K}: {got[3]}, cells with samples {(got[0] > 0).sum()}, finite minima {np.isfinite(got[2]).sum()}")
            assert v.status.shape == (n_az, m) and got[3]["n_samples"] == n_az * m
            mm.assert_same(got, want, f"{name} {n_az} x {m} K={K}")
            binned, seen = binned + got[3]["n_binned"], seen + got[3]["n_seen"]
    assert binned > 0 and 0 < seen < binned


CALL = (0.0, 360.0 / 64, 64, 30_000.0, 0.0, FAN, 128)  # 64 azimuths all around, 300 samples each


def test_grids(gpu_ctx):
    """Three grids over one viewshed, each chosen for a condition it asserts: thousands of samples in one cell (one address under every
    lane's atomics), a 3-arcsecond grid (most cells empty, some with seen and unseen samples), and a grid that leaves samples outside."""
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    pos = cfg.params.position
    coarse = generators.GeoGrid(pos.latitude - 0.5, pos.longitude - 0.5, 0.5, 0.5, 2, 2)
    fine = observer_grid(cfg, 30_000.0, 3.0 / 3600.0)
    quadrant = generators.GeoGrid(pos.latitude, pos.longitude, 0.01, 0.01, 40, 40)
    maps = {}
    for tag, grid in (("coarse 2 x 2", coarse), ("3 arcseconds", fine), ("north-east quadrant", quadrant)):
        v, want = expected(gpu_ctx, grid, CALL)
        got = to_host(fused(gpu_ctx, grid, CALL))
        work = generators.viewshed_work(gpu_ctx)
        print(f"viewshed map {tag}: {grid.n_lat} x {grid.n_lon} cells, {got[3]}, largest count {got[0].max()}, empty cells {(got[0] == 0).sum()}, "
              f"cells partly seen {((got[1] > 0) & (got[1] < got[0])).sum()}, {work}")
        mm.assert_same(got, want, tag)
        assert not work["table_rebuilt"]  # the viewshed call before it built the table under the same key
        maps[tag] = got
    assert maps["coarse 2 x 2"][0].max() >= 1000
    n_samples, n_seen = maps["3 arcseconds"][:2]
    assert (n_samples == 0).any() and ((n_seen > 0) & (n_seen < n_samples)).any()
    st = maps["north-east quadrant"][3]
    assert st["n_outside"] > 0 and st["n_binned"] > 0 and st["n_skipped"] == 0


def timings_hold(work, found):
    """every interval of the call's timing array is a finite time; after a call that found its path table the table's entry is exactly 0"""
    ms = [v for k, v in work.items() if k.endswith("_ms")]
    assert all(np.isfinite(v) and v >= 0.0 for v in ms), work
    if found:
        assert work["paths_ms"] == 0.0 and not work["table_rebuilt"], work


def test_batches(gpu_ctx, monkeypatch):
    """The scratch limit lowered until the fused call takes several batches: the same bytes as in one batch."""
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    A, tile, _ = shape()
    n_az, m = 4 * A + 1, tile + 1
    call = (0.0, 20.0, n_az, m * STEP, 10.0, FAN, 128)
    grid = observer_grid(cfg, m * STEP, 30.0 / 3600.0)
    _, want = expected(gpu_ctx, grid, call)
    whole = to_host(fused(gpu_ctx, grid, call))
    assert generators.viewshed_work(gpu_ctx)["batches"] == 1
    timings_hold(generators.viewshed_work(gpu_ctx), True)  # the viewshed of `expected` built the table under the same key
    mm.assert_same(whole, want, "one batch")
    # one azimuth adds its profile (three doubles per sample and a kilobyte) and 25 bytes per cell, some 4.2 kB here: four to a batch
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", "20000")
    split = to_host(fused(gpu_ctx, grid, call))
    work = generators.viewshed_work(gpu_ctx)
    print(f"viewshed map batches: limit 20000 bytes: {work}")
    batches = pm.batches(pm.uniform(n_az, m, 20000, pm.viewshed_map_staged(m)))
    assert 3 <= batches < n_az and work["batches"] == batches and work["download_ms"] > 0.0  # the last entry: the scatter
    timings_hold(work, True)
    monkeypatch.setenv("ATMRT_SIGHT_SCRATCH_BYTES", "1")  # a batch holds at least one azimuth
    single = to_host(fused(gpu_ctx, grid, call))
    assert generators.viewshed_work(gpu_ctx)["batches"] == n_az
    timings_hold(generators.viewshed_work(gpu_ctx), True)
    host = to_host(generators.viewshed_map(gpu_ctx, grid, *call))
    assert generators.viewshed_work(gpu_ctx)["batches"] == n_az
    assert same_bytes(whole, split) and same_bytes(whole, single) and same_bytes(whole, host)


def test_routes_give_the_same_bytes(gpu_ctx):
    """The fused device route, the host route, and the planes route fed with atmrt_viewshed_device's planes."""
    import torch
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    A, tile, two = shape()
    n_az, reach = A + 2, (tile + 5) * STEP
    dev = device(gpu_ctx)
    grid = observer_grid(cfg, reach, 15.0 / 3600.0)
    for K in (64, two):
        call = (45.0, 31.0, n_az, reach, 5.0, FAN, K)
        v, want = expected(gpu_ctx, grid, call)
        m = v.d.size - 1
        spec = _abi.ViewshedSpec(45.0, 31.0, reach, 5.0, FAN[0], FAN[1], n_az, K)
        planes = {"k_star": torch.empty((n_az, m), dtype=torch.int16, device=dev), "status": torch.empty((n_az, m), dtype=torch.uint8, device=dev),
                  "hidden": torch.empty((n_az, m), dtype=torch.float64, device=dev), "lat": torch.empty((n_az, m), dtype=torch.float64, device=dev),
                  "lon": torch.empty((n_az, m), dtype=torch.float64, device=dev)}
        gpu_ctx.check(gpu_ctx.lib.atmrt_viewshed_device(gpu_ctx.handle, C.byref(spec), planes["k_star"].data_ptr(), planes["status"].data_ptr(),
                                                        planes["hidden"].data_ptr(), None, None, planes["lat"].data_ptr(), planes["lon"].data_ptr()))
        by_planes = to_host(generators.viewshed_map_planes(gpu_ctx, grid, planes["status"], planes["hidden"], planes["lat"], planes["lon"]))
        by_device = to_host(fused(gpu_ctx, grid, call))
        by_host = to_host(generators.viewshed_map(gpu_ctx, grid, *call))
        print(f"viewshed map routes K={K}: {by_device[3]}")
        for tag, got in (("planes", by_planes), ("device", by_device), ("host", by_host)):
            mm.assert_same(got, want, f"{tag} route K={K}")
        assert same_bytes(by_device, by_host) and same_bytes(by_device, by_planes)
    # min_hidden is optional on every route: the counts are the same without it, and nothing is written through a NULL
    st = _abi.ViewshedMapStats()
    ns, nv = np.zeros((grid.n_lat, grid.n_lon), np.uint32), np.zeros((grid.n_lat, grid.n_lon), np.uint32)
    gpu_ctx.check(gpu_ctx.lib.atmrt_viewshed_map(gpu_ctx.handle, C.byref(spec), C.byref(grid), 0, ns.ctypes.data, nv.ctypes.data, None, C.byref(st)))
    assert np.array_equal(ns, want[0]) and np.array_equal(nv, want[1]) and st.n_binned == want[3]["n_binned"]
    t = generators.viewshed_map_tensors(grid, dev)
    gpu_ctx.check(gpu_ctx.lib.atmrt_viewshed_map_device(gpu_ctx.handle, C.byref(spec), C.byref(grid), 0, t["n_samples"].data_ptr(), t["n_seen"].data_ptr(), None, None))
    assert np.array_equal(t["n_samples"].cpu().numpy().view(np.uint32), want[0])


OBSERVERS = [dict(lat=46.5, lon=8.5, altitude=50.0), dict(lat=46.545, lon=8.5, altitude=50.0)]  # 5 km apart, 50 m above their ground


def test_accumulate_and_cumulative(gpu_ctx):
    """Observers A then B accumulated = the cell-wise sum and minimum of their separate maps; cumulative_viewshed counts the observers
    that see a cell."""
    import torch
    cfg, tiles = scene()
    gen = configure(gpu_ctx, cfg, tiles)
    call = (0.0, 11.25, 32, 12_000.0, 2.0, FAN, 128)
    a, b = (generators.viewshed_map_grid(o["lat"], o["lon"], 12_000.0, 15.0 / 3600.0) for o in OBSERVERS)
    cell = 15.0 / 3600.0
    grid = generators.snap_grid((min(a.lat0, b.lat0), max(g.lat0 + (g.n_lat - 0.5) * cell for g in (a, b)),
                                 min(a.lon0, b.lon0), max(g.lon0 + (g.n_lon - 0.5) * cell for g in (a, b))), cell)  # holds both observers' grids
    pos = gen.params.pod.position
    assert pos.altitude_kind == _abi.ALT_RELATIVE
    separate, device_maps = [], []
    acc = generators.viewshed_map_tensors(grid, device(gpu_ctx))
    host_acc = None
    for n, o in enumerate(OBSERVERS):
        pos.latitude, pos.longitude, pos.altitude = o["lat"], o["lon"], o["altitude"]
        gen._configure()
        _, want = expected(gpu_ctx, grid, call)
        separate.append(want)
        got = generators.viewshed_map(gpu_ctx, grid, *call, accumulate=n > 0, into=acc)
        assert got.stats == want[3]  # of this call only, also under accumulate
        host_acc = generators.viewshed_map(gpu_ctx, grid, *call, accumulate=n > 0, into=host_acc)
        assert host_acc.stats == want[3]
    pos.latitude, pos.longitude, pos.altitude = OBSERVERS[0]["lat"], OBSERVERS[0]["lon"], OBSERVERS[0]["altitude"]
    (sa, va, ma, _), (sb, vb, mb, stb) = separate
    both = to_host(generators.ViewshedMap(grid, acc["n_samples"], acc["n_seen"], acc["min_hidden"], stb))
    overlap = int(((sa > 0) & (sb > 0)).sum())
    print(f"viewshed map accumulate: {grid.n_lat} x {grid.n_lon} cells, A {separate[0][3]}, B {stb}, cells both reach {overlap}")
    assert overlap > 0 and separate[0][3]["n_outside"] == 0 and stb["n_outside"] == 0
    mm.assert_same(both, (sa + sb, va + vb, np.minimum(ma, mb), stb), "A then B")
    mm.assert_same(to_host(host_acc), (sa + sb, va + vb, np.minimum(ma, mb), stb), "A then B, host route")
    seeing, minh = generators.cumulative_viewshed(gen, OBSERVERS, grid, *call)
    want_seeing = (va > 0).astype(np.uint32) + (vb > 0).astype(np.uint32)
    got_seeing = seeing.cpu().numpy().view(np.uint32)
    print(f"viewshed map cumulative: cells seen by 0/1/2 observers {np.bincount(got_seeing.ravel(), minlength=3).tolist()}")
    assert np.array_equal(got_seeing, want_seeing) and (want_seeing == 2).any() and (want_seeing == 1).any()
    assert minh.cpu().numpy().tobytes() == np.minimum(ma, mb).tobytes()
    assert (pos.latitude, pos.longitude) == (46.5, 8.5)  # the generator's own position is back


def test_hand_made_planes(gpu_ctx):
    """The planes route on values no viewshed writes: a NaN lat, a negative hidden, status 7, +0.0 beside 5e-324, -0.0, NaN hidden, +inf."""
    import torch
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    dev = device(gpu_ctx)
    grid = generators.GeoGrid(10.0, 20.0, 1.0, 1.0, 2, 3)
    tiny = 5e-324
    rows = [  # status, hidden, lat, lon
        (vm.SEEN, 3.0, 10.5, 20.5), (vm.HIDDEN, 2.0, 10.5, 20.5), (vm.SEEN, -1.0, 10.5, 20.5),      # cell 0: the negative one is counted, not minimised
        (vm.SEEN, tiny, 10.5, 21.5), (vm.HIDDEN, 0.0, 10.5, 21.5),                                  # cell 1: +0.0 beside 5e-324 -> +0.0
        (vm.HIDDEN, tiny, 10.5, 22.5), (vm.SEEN, -0.0, 10.5, 22.5), (vm.SEEN, np.nan, 10.5, 22.5),  # cell 2: -0.0 and NaN take no part -> 5e-324
        (vm.BELOW_FAN, 0.5, 11.5, 20.5), (vm.ABOVE_FAN, np.nan, 11.5, 20.5),                       # cell 3: counted, seen once, no minimum -> +inf
        (vm.SEEN, np.inf, 11.5, 21.5),                                                              # cell 4: +inf takes part and changes nothing
        (vm.SEEN, 1.0, np.nan, 20.5), (vm.SEEN, 1.0, 10.5, np.nan), (7, 1.0, 10.5, 20.5), (4, 1.0, 11.5, 22.5),  # skipped
        (vm.SEEN, 1.0, 12.0, 20.5), (vm.SEEN, 1.0, 10.5, 23.0), (vm.SEEN, 1.0, 9.999, 20.5), (vm.SEEN, 1.0, np.inf, 20.5),  # outside: the north and east edges
        (vm.SEEN, 7.0, 10.0, 20.0),                                                                 # the south-west corner itself: cell 0
    ]
    rows = rows + rows[:3] * 90  # 290 samples: more than one block, the last wavefront partly empty
    status = np.array([r[0] for r in rows], dtype=np.uint8)
    hidden, lat, lon = (np.array([r[k] for r in rows], dtype=np.float64) for k in (1, 2, 3))
    want = mm.bin_planes(grid, status, hidden, lat, lon)
    t = [torch.from_numpy(a).to(dev) for a in (status, hidden, lat, lon)]
    got = to_host(generators.viewshed_map_planes(gpu_ctx, grid, *t))
    print(f"viewshed map hand-made: {got[3]}\n{got[0]}\n{got[1]}\n{got[2]}")
    mm.assert_same(got, want, "hand-made")
    assert got[3] == dict(n_samples=290, n_binned=282, n_outside=4, n_skipped=4, n_seen=8 + 180)
    assert got[0].tolist() == [[274, 2, 3], [2, 1, 0]] and got[1].tolist() == [[183, 1, 2], [1, 1, 0]]
    bits = got[2].view(np.uint64).tolist()
    assert bits == [[np.float64(2.0).view(np.uint64), 0, 1], [0x7FF0000000000000] * 3]
    # accumulate onto it: the counts double, the minimum stays; n = 0 leaves a map alone and clears one without accumulate
    into = dict(n_samples=torch.from_numpy(got[0].view(np.int32)).to(dev), n_seen=torch.from_numpy(got[1].view(np.int32)).to(dev),
                min_hidden=torch.from_numpy(got[2]).to(dev))
    twice = to_host(generators.viewshed_map_planes(gpu_ctx, grid, *t, accumulate=True, into=into))
    mm.assert_same(twice, mm.bin_planes(grid, status, hidden, lat, lon, into=want[:3]), "hand-made twice")
    none = [a[:0] for a in t]
    kept = to_host(generators.viewshed_map_planes(gpu_ctx, grid, *none, accumulate=True, into=into))
    assert same_bytes(kept[:3] + (0,), twice[:3] + (0,)) and kept[3] == dict.fromkeys(mm.STATS, 0)
    cleared = to_host(generators.viewshed_map_planes(gpu_ctx, grid, *none, into=into))
    assert not cleared[0].any() and not cleared[1].any() and np.isposinf(cleared[2]).all()


def test_repeatability_and_refusals(gpu_ctx):
    import torch
    cfg, tiles = scene()
    configure(gpu_ctx, cfg, tiles)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    dev = device(gpu_ctx)
    call = (10.0, 5.0, 6, 7_000.0, 0.0, FAN, 128)
    grid = observer_grid(cfg, 7_000.0, 15.0 / 3600.0)
    first = to_host(fused(gpu_ctx, grid, call))
    again = to_host(fused(gpu_ctx, grid, call))
    assert same_bytes(first, again) and first[3]["n_binned"] == 6 * 70
    # a second call that changes only the grid finds the path table
    other = generators.GeoGrid(grid.lat0, grid.lon0, 2 * grid.cell_lat, 2 * grid.cell_lon, grid.n_lat, grid.n_lon)
    fused(gpu_ctx, other, call)
    work = generators.viewshed_work(gpu_ctx)
    print(f"viewshed map, another grid: {work}")
    assert not work["table_rebuilt"] and work["paths_ms"] == 0.0 and work["batches"] == 1

    good = dict(az_lo_deg=0.0, az_step_deg=1.0, reach=1_000.0, height=0.0, fan_lo_deg=-1.0, fan_hi_deg=1.0, n_az=2, fan_rays=64)
    good_grid = (grid.lat0, grid.lon0, grid.cell_lat, grid.cell_lon, 4, 4)
    t = dict(n_samples=torch.full((4, 4), 77, dtype=torch.int32, device=dev), n_seen=torch.full((4, 4), 77, dtype=torch.int32, device=dev),
             min_hidden=torch.full((4, 4), 77.0, dtype=torch.float64, device=dev))
    a = dict(n_samples=np.full((4, 4), 77, np.uint32), n_seen=np.full((4, 4), 77, np.uint32), min_hidden=np.full((4, 4), 77.0))
    samples = dict(status=torch.zeros(8, dtype=torch.uint8, device=dev), hidden=torch.zeros(8, dtype=torch.float64, device=dev),
                   lat=torch.zeros(8, dtype=torch.float64, device=dev), lon=torch.zeros(8, dtype=torch.float64, device=dev))

    def call_map(route, handle=h, spec=True, g=good_grid, missing=(), **over):
        s = _abi.ViewshedSpec(**dict(good, **over))
        gg = None if g is None else C.byref(_abi.GeoGrid(*g))
        if route == "planes":
            ptr = [None if k in missing else v.data_ptr() for k, v in samples.items()]
            out = [None if k in missing else t[k].data_ptr() for k, _ in mm.PLANES]
            rc = lib.atmrt_viewshed_map_planes_device(handle, gg, 8, *ptr, 0, *out, None)
        else:
            out = [None if k in missing else (t[k].data_ptr() if route == "device" else a[k].ctypes.data) for k, _ in mm.PLANES]
            fn = lib.atmrt_viewshed_map_device if route == "device" else lib.atmrt_viewshed_map
            rc = fn(handle, C.byref(s) if spec else None, gg, 0, *out, None)
        return rc, lib.atmrt_last_error(handle).decode()

    untouched = lambda: all((v == 77).all().item() for v in t.values()) and all((v == 77).all() for v in a.values())
    bad_grids = [None, (np.nan, 0.0, 1.0, 1.0, 4, 4), (0.0, np.inf, 1.0, 1.0, 4, 4), (0.0, 0.0, 0.0, 1.0, 4, 4), (0.0, 0.0, 1.0, -1.0, 4, 4),
                 (0.0, 0.0, np.inf, 1.0, 4, 4), (0.0, 0.0, 1.0, 1.0, 0, 4), (0.0, 0.0, 1.0, 1.0, 4, 0), (0.0, 0.0, 1.0, 1.0, 65536, 65536)]
    for g in bad_grids:  # a grid atmrt_geo_grid_cell refuses
        if g is not None:
            assert lib.atmrt_geo_grid_cell(C.byref(_abi.GeoGrid(*g)), 0.5, 0.5, C.byref(C.c_int64())) == _abi.ERR_INVALID_ARGUMENT, g
        for route in ("device", "host", "planes"):
            rc, msg = call_map(route, g=g)
            assert rc == _abi.ERR_INVALID_ARGUMENT and msg, (route, g, rc, msg)
    bad_specs = [dict(spec=False), dict(az_lo_deg=np.nan), dict(az_step_deg=np.inf), dict(az_lo_deg=1e308, az_step_deg=1e308), dict(reach=0.0), dict(reach=-1.0),
                 dict(reach=np.nan), dict(reach=np.inf), dict(reach=65_536 * STEP), dict(height=-1.0), dict(height=np.nan), dict(n_az=0), dict(n_az=-3),
                 dict(n_az=65_537), dict(fan_rays=0), dict(fan_rays=63), dict(fan_rays=96), dict(fan_rays=4160), dict(fan_lo_deg=np.nan), dict(fan_hi_deg=np.inf),
                 dict(fan_lo_deg=1.0, fan_hi_deg=1.0), dict(fan_lo_deg=2.0, fan_hi_deg=1.0), dict(fan_lo_deg=-91.0, fan_hi_deg=90.0),
                 dict(reach=65_535 * STEP, fan_rays=4096, n_az=1)]  # everything atmrt_viewshed refuses in a spec
    for kw in bad_specs:
        for route in ("device", "host"):
            rc, msg = call_map(route, **kw)
            assert rc == _abi.ERR_INVALID_ARGUMENT and msg, (route, kw, rc, msg)
    for route in ("device", "host", "planes"):  # a NULL required plane; min_hidden is not one
        for k in ("n_samples", "n_seen"):
            assert call_map(route, missing=(k,))[0] == _abi.ERR_INVALID_ARGUMENT, (route, k)
    for k in samples:
        assert call_map("planes", missing=(k,))[0] == _abi.ERR_INVALID_ARGUMENT, k
    assert untouched()  # refused before any plane is touched
    fresh = generators.Context(gpu_ctx.device)
    try:
        for route in ("device", "host", "planes"):
            rc, msg = call_map(route, handle=fresh.handle)
            assert rc == _abi.ERR_STATE and "atmrt_set_params" in msg, (route, rc, msg)
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        pod = _abi.Params.from_buffer_copy(cfg.params)
        multi.check(lib.atmrt_set_params(multi.handle, C.byref(pod)))
        for route in ("device", "host", "planes"):
            rc, msg = call_map(route, handle=multi.handle)
            assert rc == _abi.ERR_STATE and "multi-device" in msg, (route, rc, msg)
    finally:
        multi.close()
    assert untouched()
    for route in ("device", "host", "planes"):
        assert call_map(route)[0] == 0 and call_map(route, missing=("min_hidden",))[0] == 0, route
    # the context still answers a plain viewshed, and the same map as before
    v = generators.viewshed(gpu_ctx, *call)
    assert v.status.shape == (6, 70)
    mm.assert_same(to_host(fused(gpu_ctx, grid, call)), mm.bin_planes(grid, v.status, v.hidden, v.lat, v.lon), "after the refusals")


def test_gen_viewshed_map(gpu_ctx, tmp_path):
    """`gen --viewshed-map OUT.npz` end to end: the arrays equal generators.viewshed_map for the same call, and n_samples sums to the
    stats' n_binned; the cumulative form through the same function the command calls."""
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 90.0, "fov": 30.0, "tilt": 0.0, "max_distance": 9_000.0}},
           "simulation_step": 100.0, "output": {"width": 48, "height": 32, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--viewshed-map", "map.npz", "--map-cell", "6",
                        "--viewshed-az", "0", "350", "36", "--viewshed-reach", "6450", "--viewshed-height", "12.5", "--viewshed-fan", "-4", "3", "128"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from atm_raytracer_amd import config
    from atm_raytracer_amd.__main__ import write_viewshed_map
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    gen = generators.make_generator(generators.Params(cfg), terrain)
    gen._configure()
    grid = generators.viewshed_map_grid(46.5, 8.5, 6_500.0, 6.0 / 3600.0)
    want = generators.viewshed_map(gpu_ctx, grid, 0.0, 10.0, 36, 6_450.0, 12.5, (-4.0, 3.0), 128)
    with np.load(tmp_path / "map.npz") as z:
        assert set(z.files) == {"n_samples", "n_seen", "min_hidden", "lat0", "lon0", "cell_lat", "cell_lon", "n_lat", "n_lon"} | {"stats_" + k for k in mm.STATS}
        assert [float(z[k]) for k in ("lat0", "lon0", "cell_lat", "cell_lon")] == [grid.lat0, grid.lon0, grid.cell_lat, grid.cell_lon]
        assert (int(z["n_lat"]), int(z["n_lon"])) == (grid.n_lat, grid.n_lon) == z["n_samples"].shape
        for k, t in mm.PLANES:
            assert z[k].dtype == t and z[k].tobytes() == getattr(want, k).tobytes(), k
        print(f"gen --viewshed-map: {grid.n_lat} x {grid.n_lon} cells, {want.stats}")
        assert int(z["n_samples"].sum()) == int(z["stats_n_binned"]) == want.stats["n_binned"] == 36 * 65 and int(z["stats_n_outside"]) == 0
    (tmp_path / "observers.csv").write_text("lat,lon,altitude\n46.5,8.5,50\n46.52,8.53,80\n")
    seeing, minh = write_viewshed_map(gpu_ctx, cfg, gen, str(tmp_path / "cum.npz"), 6.0, (0.0, 350.0, 36), 6_450.0, 12.5, (-4.0, 3.0, 128), str(tmp_path / "observers.csv"))
    with np.load(tmp_path / "cum.npz") as z:
        assert set(z.files) == {"observers_seeing", "min_hidden", "lat0", "lon0", "cell_lat", "cell_lon", "n_lat", "n_lon"}
        assert z["observers_seeing"].dtype == np.uint32 and z["observers_seeing"].tobytes() == seeing.tobytes() and z["min_hidden"].tobytes() == minh.tobytes()
        cum_grid = generators.GeoGrid(float(z["lat0"]), float(z["lon0"]), float(z["cell_lat"]), float(z["cell_lon"]), int(z["n_lat"]), int(z["n_lon"]))
    # the first observer is the configured one: where its own map sees ground the cumulative count is at least one
    own = generators.viewshed_map(gpu_ctx, cum_grid, 0.0, 10.0, 36, 6_450.0, 12.5, (-4.0, 3.0), 128)
    assert own.stats["n_outside"] == 0 and (seeing[own.n_seen > 0] >= 1).all() and seeing.max() == 2 and (seeing <= 2).all()
