"""atmrt_shadow_mask* and atmrt_draw_image_shadowed on the GPU against tests/shadow_model.py (the rule of include/atmrt.h over the
oracle's coords_at_dist, get_elev and ray stepper): status and block byte for byte, the call's counts, and the shadowed image against
oracle.draw_image over the model's result.  The frames and specs are tests/shadow_cases.py's; tests/test_shadow_model.py asserts
without a GPU that each of them holds both kinds of pixel.  Every case prints its figures before it asserts (`shadow <case>: ...`)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shadow_cases as sc
import shadow_model as sm
from atm_raytracer_amd import _abi, generators
from util import run_gpu

pytestmark = pytest.mark.gpu

SHADING = dict(kind=1, water_level=300.0, ambient_light=0.3, light_zenith_angle=88.0, light_dir=190.0, palette=1, has_fog=0, fog_distance=30_000.0)


def shading_for(cfg, spec, **over):
    """The Shading configuration whose light is the spec's (generators.light_from_coloring read backwards): the slopes that face the
    light are bright in the plain image, so a cast shadow on them shows."""
    return dict(SHADING, light_zenith_angle=90.0 - spec[1], light_dir=cfg.params.frame.direction + 180.0 - spec[0], **over)


@pytest.fixture(scope="module")
def models(oracle_det):
    """The model's answer per case, computed once from the frame the GPU generated and shared by the tests below."""
    made, settings = {}, {}

    def get(name, cfg, tiles, res):
        if name not in made:
            frame = sc.CASES[name][0]
            if frame not in settings:
                settings[frame] = sm.Setting(oracle_det, cfg, tiles)
            made[name] = sm.solve(settings[frame], res, sc.CASES[name][1])
        return made[name]

    yield get
    for s in settings.values():
        s.close()


def frame_of(ctx, name):
    """The case's frame generated on the context -> (cfg, tiles, result, spec)."""
    frame, spec, _ = sc.CASES[name]
    cfg, tiles = sc.FRAMES[frame]()
    return cfg, tiles, run_gpu(ctx, cfg, tiles), spec


def assert_mask(got, want, stats, tag):
    for k in ("status", "block"):
        g, w = getattr(got, k), getattr(want, k)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{tag} {k}: {bad.size} of {g.size} differ, first at {bad[:5]}: {g.ravel()[bad[:5]]} vs {w.ravel()[bad[:5]]}"
    assert got.stats == stats, (tag, got.stats, stats)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_mask_equals_the_model(gpu_ctx, models, name):
    cfg, tiles, res, spec = frame_of(gpu_ctx, name)
    W, H = res["width"], res["height"]
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, SHADING)
    before = generators.draw_image(gpu_ctx, coloring, W, H)
    got = generators.shadow_mask(gpu_ctx, spec, W, H)
    want = models(name, cfg, tiles, res)
    t = generators.shadow_timings(gpu_ctx)
    print(f"shadow {name}: {W}x{H} m={want.m} stats={got.stats} model={want.stats_on} floor={want.floor:g} "
          f"compact {t['compact_ms']:.3f} march {t['march_ms']:.3f} download {t['download_ms']:.3f} ms")
    assert generators.shadow_steps(gpu_ctx, spec[2]) == want.m == 200
    assert_mask(got, want, want.stats_on, name)
    assert got.stats["none"] + got.stats["lit"] + got.stats["shadowed"] == W * H
    # two calls: the same bytes; without the block plane: the same status
    again = generators.shadow_mask(gpu_ctx, spec, W, H)
    assert again.status.tobytes() == got.status.tobytes() and again.block.tobytes() == got.block.tobytes() and again.stats == got.stats
    alone = generators.shadow_mask(gpu_ctx, spec, W, H, block=False)
    assert alone.block is None and alone.status.tobytes() == got.status.tobytes() and alone.stats == got.stats
    # the frame is intact
    assert generators.draw_image(gpu_ctx, coloring, W, H).tobytes() == before.tobytes()
    frame = sc.CASES[name][0]
    if frame == "sky":
        assert not got.status.any() and not got.block.any() and got.stats == dict(none=W * H, lit=0, shadowed=0, integrated_steps=0, escaped_rays=0)
    else:
        hit = W * H - got.stats["none"]
        assert got.stats["lit"] >= 0.05 * hit and got.stats["shadowed"] >= 0.05 * hit
    if frame == "ground":
        assert got.stats["none"] == 0
    if frame == "flat_distorted":
        assert got.stats["escaped_rays"] == 0 and want.floor == math.inf
    if frame == "alpha":
        assert (res["hit_count"] > 1).any() and (res["hit_offset"].ravel()[1:] != np.arange(1, W * H)).any()  # packed lists
    if frame == "objects":
        first = res["hit_offset"].ravel()[res["hit_count"].ravel() > 0].astype(np.int64)
        assert (res["color_tag"][first] == _abi.COLOR_RGBA).any()  # objects receive shadows


def test_lift_changes_the_answer(gpu_ctx, models):
    """lift 0 and 2 m over the same frame: both equal the model (above), and they differ."""
    cfg, tiles, res, _ = frame_of(gpu_ctx, "rect")
    a = models("rect", cfg, tiles, res)
    b = models("rect_lift2", cfg, tiles, res)
    print(f"shadow lift: shadowed {a.stats_on['shadowed']} at 0 m, {b.stats_on['shadowed']} at 2 m")
    assert a.status.tobytes() != b.status.tobytes() and b.stats_on["shadowed"] < a.stats_on["shadowed"]


@pytest.mark.parametrize("name", [n for n in sorted(sc.CASES) if sc.CASES[n][2]])
def test_escape_shortcut_off_equals_on(gpu_ctx, models, monkeypatch, name):
    cfg, tiles, res, spec = frame_of(gpu_ctx, name)
    W, H = res["width"], res["height"]
    want = models(name, cfg, tiles, res)
    on = generators.shadow_mask(gpu_ctx, spec, W, H)
    monkeypatch.setenv("ATMRT_SHADOW_ESCAPE", "off")
    off = generators.shadow_mask(gpu_ctx, spec, W, H)
    monkeypatch.delenv("ATMRT_SHADOW_ESCAPE")
    print(f"shadow escape {name}: on {on.stats}, off {off.stats}")
    assert_mask(on, want, want.stats_on, name + " on")
    assert_mask(off, want, want.stats_off, name + " off")
    assert off.stats["integrated_steps"] > on.stats["integrated_steps"] and on.stats["escaped_rays"] > 0 and off.stats["escaped_rays"] == 0


def test_device_entry_points_equal_the_frame_call(gpu_ctx):
    """atmrt_shadow_mask_device, and atmrt_shadow_mask_planes_device over the frame's first trace points downloaded and uploaded
    again: the bytes and counts of atmrt_shadow_mask.  Translucent terrain: the frame call reads the lists, the planes call planes."""
    cfg, tiles, res, spec_t = frame_of(gpu_ctx, "alpha")
    W, H = res["width"], res["height"]
    host = generators.shadow_mask(gpu_ctx, spec_t, W, H)
    spec = generators.shadow_spec(*spec_t)
    lib, st = gpu_ctx.lib, _abi.ShadowStats()
    status = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    block = torch.full((H, W), 77, dtype=torch.int16, device="cuda")
    gpu_ctx.check(lib.atmrt_shadow_mask_device(gpu_ctx.handle, C.byref(spec), status.data_ptr(), block.data_ptr(), C.byref(st)))
    assert status.cpu().numpy().tobytes() == host.status.tobytes() and block.cpu().numpy().tobytes() == host.block.tobytes()
    assert generators._shadow_stats(st) == host.stats
    hit = res["hit_count"] > 0
    first = res["hit_offset"][hit].astype(np.int64)
    planes = {}
    for k in ("lat", "lon", "elevation"):
        a = np.full((H, W), np.nan)
        a[hit] = res[k][first]
        planes[k] = torch.from_numpy(a).cuda()
    count = torch.from_numpy(res["hit_count"].astype(np.int32)).cuda()
    status2 = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    block2 = torch.full((H, W), 77, dtype=torch.int16, device="cuda")
    st2 = _abi.ShadowStats()
    gpu_ctx.check(lib.atmrt_shadow_mask_planes_device(gpu_ctx.handle, C.byref(spec), W * H, count.data_ptr(), planes["lat"].data_ptr(),
                                                      planes["lon"].data_ptr(), planes["elevation"].data_ptr(), status2.data_ptr(),
                                                      block2.data_ptr(), C.byref(st2)))
    print(f"shadow planes: {generators._shadow_stats(st2)}")
    assert torch.equal(status2, status) and torch.equal(block2, block) and generators._shadow_stats(st2) == host.stats
    # block and stats are optional
    status3 = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    gpu_ctx.check(lib.atmrt_shadow_mask_planes_device(gpu_ctx.handle, C.byref(spec), W * H, count.data_ptr(), planes["lat"].data_ptr(),
                                                      planes["lon"].data_ptr(), planes["elevation"].data_ptr(), status3.data_ptr(), None, None))
    assert torch.equal(status3, status)


@pytest.mark.parametrize("name", ["rect", "alpha", "objects"])
def test_shadowed_image_equals_the_oracle(gpu_ctx, oracle_det, models, name):
    """Under Shading, both palettes, with and without fog: oracle.draw_image over the frame with the first normals of the SHADOWED
    pixels zeroed, byte for byte, through the host and the device entry point; under Simple: the unshadowed image."""
    cfg, tiles, res, spec = frame_of(gpu_ctx, name)
    W, H = res["width"], res["height"]
    mask = generators.shadow_mask(gpu_ctx, spec, W, H)
    want_mask = models(name, cfg, tiles, res)
    assert mask.status.tobytes() == want_mask.status.tobytes()
    expected_frame = sm.shadowed_result(res, mask.status)
    for palette in (0, 1):
        for fog in (0, 1):
            conf = shading_for(cfg, spec, palette=palette, has_fog=fog)
            coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, conf)
            plain = generators.draw_image(gpu_ctx, coloring, W, H)
            got = generators.draw_image(gpu_ctx, coloring, W, H, shadows=mask.status)
            want = oracle_det.draw_image(expected_frame, oracle_det.into_coloring(cfg.params, conf))
            differ = int((got != plain).any(axis=2).sum())
            print(f"shadow draw {name} palette {palette} fog {fog}: {differ} of {W * H} pixels differ from the plain image, {int((mask.status == 2).sum())} shadowed")
            assert got.tobytes() == want.tobytes(), np.argwhere((got != want).any(axis=2))[:5]
            assert plain.tobytes() == oracle_det.draw_image(res, oracle_det.into_coloring(cfg.params, conf)).tobytes()
            assert differ >= 1
            assert not (got != plain).any(axis=2)[mask.status != 2].any()  # only SHADOWED pixels change
            d_status = torch.from_numpy(mask.status).cuda()
            d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            gpu_ctx.check(gpu_ctx.lib.atmrt_draw_image_shadowed_device(gpu_ctx.handle, C.byref(coloring), d_status.data_ptr(), d_rgb.data_ptr()))
            assert d_rgb.cpu().numpy().tobytes() == want.tobytes()
    simple = generators.into_coloring(gpu_ctx.lib, cfg.params, dict(SHADING, kind=0))
    assert generators.draw_image(gpu_ctx, simple, W, H, shadows=mask.status).tobytes() == generators.draw_image(gpu_ctx, simple, W, H).tobytes()


def test_steps_against_the_models_lattice(gpu_ctx):
    cfg, tiles, res, _ = frame_of(gpu_ctx, "fast")
    for reach in (40.0, 100.0, 100.0000001, 300.0, 19_999.0, 20_000.0, 20_000.5, 6_553_500.0):
        assert generators.shadow_steps(gpu_ctx, reach) == sm.lattice(sc.STEP, reach)[1], reach
    assert generators.shadow_steps(gpu_ctx, 40.0) == 1 and generators.shadow_steps(gpu_ctx, 6_553_500.0) == 65535


def test_refusals(gpu_ctx):
    cfg, tiles, res, spec_t = frame_of(gpu_ctx, "fast")
    W, H = res["width"], res["height"]
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    status, block, rgb = np.full((H, W), 9, np.uint8), np.full((H, W), 9, np.uint16), np.zeros((H, W, 3), np.uint8)
    d_status = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    d_f64 = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    good = generators.shadow_spec(*spec_t)
    m = C.c_int32()

    def calls(ctx_handle, spec, st=status.ctypes.data):
        p = None if spec is None else C.byref(spec)
        return (lib.atmrt_shadow_mask(ctx_handle, p, st, block.ctypes.data, None),
                lib.atmrt_shadow_mask_device(ctx_handle, p, None if st is None else d_status.data_ptr(), None, None),
                lib.atmrt_shadow_mask_planes_device(ctx_handle, p, W * H, d_cnt.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(),
                                                    None if st is None else d_status.data_ptr(), None, None))

    inf, nan = math.inf, math.nan
    bad = [(nan, 2.0, 1e4, 0.0), (inf, 2.0, 1e4, 0.0), (0.0, nan, 1e4, 0.0), (0.0, 90.0, 1e4, 0.0), (0.0, -90.0, 1e4, 0.0), (0.0, 120.0, 1e4, 0.0),
           (0.0, 2.0, 0.0, 0.0), (0.0, 2.0, -5.0, 0.0), (0.0, 2.0, nan, 0.0), (0.0, 2.0, inf, 0.0), (0.0, 2.0, 1e4, -0.001), (0.0, 2.0, 1e4, nan),
           (0.0, 2.0, 1e4, inf), (0.0, 2.0, 6_553_600.0, 0.0)]  # the last: m = 65536
    for b in bad:
        assert calls(h, generators.shadow_spec(*b)) == (_abi.ERR_INVALID_ARGUMENT,) * 3, b
        assert lib.atmrt_last_error(h)
    assert calls(h, None) == (_abi.ERR_INVALID_ARGUMENT,) * 3 and calls(h, good, st=None) == (_abi.ERR_INVALID_ARGUMENT,) * 3
    assert calls(None, good) == (_abi.ERR_INVALID_ARGUMENT,) * 3
    assert (status == 9).all() and (block == 9).all()
    assert lib.atmrt_shadow_mask_planes_device(h, C.byref(good), 0, d_cnt.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_status.data_ptr(),
                                               None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_mask_planes_device(h, C.byref(good), W * H, None, d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_status.data_ptr(),
                                               None, None) == _abi.ERR_INVALID_ARGUMENT
    for reach in (0.0, -1.0, nan, inf, 6_553_600.0):
        assert lib.atmrt_shadow_steps(h, reach, C.byref(m)) == _abi.ERR_INVALID_ARGUMENT, reach
    assert lib.atmrt_shadow_steps(h, 100.0, None) == _abi.ERR_INVALID_ARGUMENT and lib.atmrt_shadow_steps(None, 100.0, C.byref(m)) == _abi.ERR_INVALID_ARGUMENT
    coloring = generators.into_coloring(lib, cfg.params, SHADING)
    assert lib.atmrt_draw_image_shadowed(h, C.byref(coloring), None, rgb.ctypes.data) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_draw_image_shadowed(h, None, status.ctypes.data, rgb.ctypes.data) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_draw_image_shadowed_device(h, C.byref(coloring), d_status.data_ptr(), None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_shadow_timings(h, None) == _abi.ERR_INVALID_ARGUMENT
    # no parameters, then parameters and no frame
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert calls(fresh.handle, good) == (_abi.ERR_STATE,) * 3 and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        assert lib.atmrt_shadow_steps(fresh.handle, 100.0, C.byref(m)) == _abi.ERR_STATE
        assert lib.atmrt_draw_image_shadowed(fresh.handle, C.byref(coloring), status.ctypes.data, rgb.ctypes.data) == _abi.ERR_STATE
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, fresh))._configure()
        rc = calls(fresh.handle, good)
        assert rc[:2] == (_abi.ERR_STATE,) * 2 and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert rc[2] == _abi.OK  # the planes call needs no frame: all NONE here (hit_count 0)
        assert not d_status.any()
        assert lib.atmrt_shadow_steps(fresh.handle, 250.0, C.byref(m)) == _abi.OK and m.value == 3
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, multi))._configure()
        assert lib.atmrt_shadow_mask(multi.handle, C.byref(good), status.ctypes.data, None, None) == _abi.ERR_STATE
        assert b"atmrt_shadow_mask_planes_device" in lib.atmrt_last_error(multi.handle)
        assert lib.atmrt_shadow_mask_device(multi.handle, C.byref(good), d_status.data_ptr(), None, None) == _abi.ERR_STATE
        assert lib.atmrt_draw_image_shadowed(multi.handle, C.byref(coloring), status.ctypes.data, rgb.ctypes.data) == _abi.ERR_STATE
    finally:
        multi.close()
