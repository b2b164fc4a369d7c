"""atmrt_sky_light_rays, atmrt_sky_light* and atmrt_sky_shade* on the GPU against tests/sky_light_model.py (the rule of
include/atmrt.h, "sky light", over the oracle's stepper and oracle_n): status, steps, the counts, the bits of the true elevation
and of the column byte for byte, all NaNs as one value; the body plane and the shaded image byte for byte.  The frames and lists
are tests/sky_light_cases.py's (tests/sky_cases.py's: sky step 1000 m, top 100 km, m = 1500); tests/test_sky_light_model.py asserts
without a GPU what each of them holds.  Every case prints its figures before it asserts (`sky light <case>: ...`)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sky_light_cases as lc
import sky_light_model as slm
from atm_raytracer_amd import _abi, config, generators, synth
from util import bits, run_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = dict(step=lc.STEP, top=lc.TOP, floor=lc.FLOOR, m=lc.M)
SIMPLE = dict(kind=0, water_level=300.0, ambient_light=0.3, light_zenith_angle=88.0, light_dir=190.0, palette=1, has_fog=0, fog_distance=30_000.0)


def assert_planes(got, want, tag, keys=("status", "steps", "true_elevation", "column")):
    for k in keys:
        g, w = bits(getattr(got, k)), bits(getattr(want, k))
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert g.dtype == w.dtype and bad.size == 0, f"{tag} {k}: {bad.size} of {g.size} differ, first at {bad[:5]}: {getattr(got, k).ravel()[bad[:5]]} vs {getattr(want, k).ravel()[bad[:5]]}"
    assert got.stats == want.stats, (tag, got.stats, want.stats)


@pytest.fixture(scope="module")
def sphere(oracle_det):
    cfg, _ = lc.FRAMES["rect"]()
    return cfg, slm.Setting.of_config(oracle_det, cfg)


@pytest.fixture(scope="module")
def frames(oracle_det):
    """The model's answer per frame, computed once from the frame the GPU generated and shared by the tests below."""
    made = {}

    def get(ctx, name):
        cfg, tiles = lc.FRAMES[name]()
        res = run_gpu(ctx, cfg, tiles)  # leaves the frame and its setting on the context
        if name not in made:
            setting = slm.Setting.of_config(oracle_det, cfg)
            made[name] = (slm.frame(setting, res, lc.H0, lc.STEP, lc.TOP, lc.FLOOR, lc.M), slm.zenith_column(setting, lc.REF_ALT, lc.TOP, lc.STEP))
        return cfg, res, made[name][0], made[name][1]

    return get


@pytest.mark.parametrize("n", lc.LIST_LENGTHS)
def test_list_call_equals_the_model(gpu_ctx, sphere, n):
    cfg, setting = sphere
    generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, gpu_ctx))._configure()
    for tag, elev, m in (("long", lc.list_elevations(n), lc.M), ("short", lc.list_elevations_short(n), lc.SHORT_M)):
        want = slm.rays(setting, lc.LIST_H0, elev, lc.STEP, lc.TOP, lc.FLOOR, m)
        rec = np.zeros(n + 2, dtype=generators.SKY_RAY_DTYPE)
        rec.view(np.uint8)[:] = 0x77  # pre-filled, and two records of guard behind the list
        column = np.full(n + 2, 77.0)
        st = _abi.SkyStats(*[77] * 6)
        spec = generators.sky_spec(lc.STEP, lc.TOP, lc.FLOOR, m)
        e = np.ascontiguousarray(elev, dtype=np.float64)
        gpu_ctx.check(gpu_ctx.lib.atmrt_sky_light_rays(gpu_ctx.handle, C.byref(spec), lc.LIST_H0, n, e.ctypes.data, rec.ctypes.data, column.ctypes.data,
                                                       C.byref(st)))
        got = slm.sm.Result()
        got.status, got.steps, got.true_elevation = rec["status"][:n].astype(np.uint8), rec["steps"][:n].copy(), rec["true_elevation"][:n].copy()
        got.column, got.stats = column[:n].copy(), generators._sky_stats(st)
        print(f"sky light list {tag} n={n}: {got.stats} {generators.sky_timings(gpu_ctx)}")
        assert (rec.view(np.uint8)[16 * n:] == 0x77).all() and (column[n:] == 77.0).all()
        assert_planes(got, want, f"list {tag} {n}")
        plain, plain_stats = generators.sky_rays(gpu_ctx, lc.LIST_H0, elev, spec=spec)  # the sky-ray call: the same records
        assert plain.tobytes() == rec[:n].tobytes() and plain_stats == got.stats
        if n >= 63 and tag == "short":
            assert {slm.GROUND, slm.EXIT, slm.INSIDE} <= set(got.status[:63].tolist())  # inside one wavefront


@pytest.mark.parametrize("name", sorted(lc.FRAMES))
def test_frame_equals_the_model(gpu_ctx, frames, monkeypatch, name):
    cfg, res, want, z0 = frames(gpu_ctx, name)
    W, H = res["width"], res["height"]
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, SIMPLE)
    before = generators.draw_image(gpu_ctx, coloring, W, H)
    got = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    t = generators.sky_timings(gpu_ctx)
    exits = got.status == slm.EXIT
    x = got.air_mass[exits]
    print(f"sky light {name}: {W}x{H} stats={got.stats} Z0 {got.zenith_column!r} air mass {x.min() if x.size else math.nan:.3f} .. "
          f"{x.max() if x.size else math.nan:.3f} compact {t['compact_ms']:.3f} march {t['march_ms']:.3f} download {t['download_ms']:.3f} ms")
    assert_planes(got, want, name)
    assert bits(np.float64(got.zenith_column)) == bits(np.float64(z0))
    # the planes of the sky-ray call, bit for bit, and its counts
    sky = generators.sky_directions(gpu_ctx, W, H, **SPEC)
    assert_planes(got, sky, name + " sky rays", keys=("status", "steps", "true_elevation"))
    assert (np.isnan(got.column) | exits).all() and sum(got.stats[k] for k in ("none", "exit", "ground", "inside", "lost")) == W * H
    if name in lc.US76_SPHERE and x.size:
        assert (x > 0.7).all() and (x < 80.0).all() and not np.isnan(got.column[exits]).any()
    # two equal calls: the same bytes; without the steps plane: the same planes; the other list order: the same bytes
    again = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    assert_planes(again, got, name + " again")
    alone = generators.sky_light(gpu_ctx, W, H, steps=False, ref_alt=lc.REF_ALT, **SPEC)
    assert alone.steps is None
    assert_planes(alone, got, name + " without steps", keys=("status", "true_elevation", "column"))
    monkeypatch.setenv("ATMRT_SKY_ORDER", "forward")
    forward = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    monkeypatch.delenv("ATMRT_SKY_ORDER")
    assert_planes(forward, got, name + " forward")
    # the frame is intact
    assert generators.draw_image(gpu_ctx, coloring, W, H).tobytes() == before.tobytes()


def test_shade_equals_the_model(gpu_ctx, frames):
    cfg, res, want, z0 = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, SIMPLE)
    plain = generators.draw_image(gpu_ctx, coloring, W, H)
    light = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    exits = light.status == slm.EXIT
    x = W // 2
    rows = np.flatnonzero(exits[:, x])
    y = int(rows[len(rows) // 2])
    sun = (float(res["azimuth"][y, x]), float(light.true_elevation[y, x]), 2.0, (255, 236, 170))  # a disc of a dozen pixels at 48 x 24
    moon = (sun[0] + 2.4, sun[1] + 0.8, 2.0, (200, 200, 220))  # overlaps the sun, its disc ends 0.5 degrees short of the sun's centre
    for tag, bodies, params in (("no body", [], {}), ("sun", [sun], {}), ("sun and moon", [sun, moon], {}), ("moon and sun", [moon, sun], {}),
                                ("saturating", [sun], dict(exposure=40.0)), ("grey, full limb", [sun, moon], dict(airlight=(120, 130, 140), exposure=1.0, limb=(1.0, 1.0, 1.0)))):
        want_body, want_image = slm.shade(plain, z0, bodies, res["azimuth"], want.true_elevation, want.status, want.column, **params)
        image = plain.copy()
        body = generators.sky_shade(gpu_ctx, light, bodies, image, **params)
        print(f"sky light shade {tag}: body pixels {np.bincount(body.ravel()).tolist()}, {generators.sky_shade_timing(gpu_ctx):.3f} ms, "
              f"zenith-most sky pixel {image[exits][0].tolist()}, centre pixel {image[y, x].tolist()}")
        assert body.dtype == np.uint8 and body.tobytes() == want_body.tobytes()
        assert body.tobytes() == generators.sky_bodies(gpu_ctx, light, bodies).tobytes()  # the body plane of atmrt_sky_bodies
        assert image.tobytes() == want_image.tobytes()
        assert (image[~exits] == plain[~exits]).all()  # the bytes of pixels that are not EXIT are untouched
        if bodies:
            assert (body != 0).sum() >= 4 and body[y, x] == bodies.index(sun) + 1  # the centre pixel is the sun's alone
        # draw_image(sky_light=) is the same image: given the SkyLight itself, or the shade's parameters beside it
        drawn = generators.draw_image(gpu_ctx, coloring, W, H, bodies=bodies, sky=light, sky_light=dict(params) if params else light)
        assert drawn.tobytes() == image.tobytes()
    drawn = generators.draw_image(gpu_ctx, coloring, W, H, sky=light, sky_light=True)
    assert drawn.tobytes() == slm.shade(plain, z0, [], res["azimuth"], want.true_elevation, want.status, want.column)[1].tobytes()


def test_device_and_planes_entry_points(gpu_ctx, frames):
    """atmrt_sky_light_device and atmrt_sky_shade_device over device planes, atmrt_sky_light_planes_device and
    atmrt_sky_shade_planes_device over the frame's own planes uploaded again with its h0: the bytes of the host-array calls, with
    guards behind every plane."""
    cfg, res, want, z0 = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    n, lib = W * H, gpu_ctx.lib
    spec = generators.sky_light_spec(lc.REF_ALT, sky=generators.sky_spec(**SPEC))
    coloring = generators.into_coloring(lib, cfg.params, SIMPLE)
    plain = generators.draw_image(gpu_ctx, coloring, W, H)
    host = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    sun = (float(res["azimuth"][2, W // 2]), float(np.nanmax(want.true_elevation[2])), 0.8, (255, 236, 170))
    host_image = plain.copy()
    host_body = generators.sky_shade(gpu_ctx, host, [sun], host_image)
    arr, nb = generators._sky_bodies_array([sun])
    shade = generators.sky_shade_params(host.zenith_column)

    def planes():
        return (torch.full((n + 8,), 77.0, dtype=torch.float64, device="cuda"), torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda"),
                torch.full((n + 8,), 77, dtype=torch.int32, device="cuda"), torch.full((n + 8,), 77.0, dtype=torch.float64, device="cuda"))

    def result(d_true, d_status, d_steps, d_column, st):
        assert (d_true[n:] == 77.0).all() and (d_status[n:] == 77).all() and (d_steps[n:] == 77).all() and (d_column[n:] == 77.0).all()
        got = slm.sm.Result()
        got.true_elevation, got.status = d_true[:n].cpu().numpy().reshape(H, W), d_status[:n].cpu().numpy().reshape(H, W)
        got.steps, got.column = d_steps[:n].cpu().numpy().view(np.uint32).reshape(H, W), d_column[:n].cpu().numpy().reshape(H, W)
        got.stats = generators._sky_stats(st)
        return got

    def shade_result(d_body, d_rgb, tag):
        assert (d_body[n:] == 77).all() and (d_rgb[3 * n:] == 77).all()
        assert d_body[:n].cpu().numpy().tobytes() == host_body.tobytes(), tag
        assert d_rgb[:3 * n].cpu().numpy().tobytes() == host_image.tobytes(), tag

    def image_planes():
        d_rgb = torch.full((3 * n + 8,), 77, dtype=torch.uint8, device="cuda")
        d_rgb[:3 * n] = torch.from_numpy(plain.ravel()).cuda()
        return torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda"), d_rgb

    d_true, d_status, d_steps, d_column = planes()
    st, z = _abi.SkyStats(), C.c_double()
    torch.cuda.synchronize()  # the fills above run on torch's stream, the library on its own
    gpu_ctx.check(lib.atmrt_sky_light_device(gpu_ctx.handle, C.byref(spec), d_true.data_ptr(), d_status.data_ptr(), d_steps.data_ptr(), d_column.data_ptr(),
                                             C.byref(st), C.byref(z)))
    torch.cuda.synchronize()
    assert_planes(result(d_true, d_status, d_steps, d_column, st), host, "device")
    assert z.value == host.zenith_column
    d_body, d_rgb = image_planes()
    torch.cuda.synchronize()
    gpu_ctx.check(lib.atmrt_sky_shade_device(gpu_ctx.handle, C.byref(shade), arr, nb, d_true.data_ptr(), d_status.data_ptr(), d_column.data_ptr(),
                                             d_body.data_ptr(), d_rgb.data_ptr()))
    torch.cuda.synchronize()
    shade_result(d_body, d_rgb, "shade device")

    d_hit = torch.from_numpy(np.ascontiguousarray(res["hit_count"], dtype=np.uint32).view(np.int32).ravel()).cuda()
    d_el = torch.from_numpy(np.ascontiguousarray(res["elevation_angle"], dtype=np.float64).ravel()).cuda()
    d_az = torch.from_numpy(np.ascontiguousarray(res["azimuth"], dtype=np.float64).ravel()).cuda()
    d_true, d_status, d_steps, d_column = planes()
    st, z = _abi.SkyStats(), C.c_double()
    torch.cuda.synchronize()
    gpu_ctx.check(lib.atmrt_sky_light_planes_device(gpu_ctx.handle, C.byref(spec), lc.H0, n, d_hit.data_ptr(), d_el.data_ptr(), d_true.data_ptr(),
                                                    d_status.data_ptr(), d_steps.data_ptr(), d_column.data_ptr(), C.byref(st), C.byref(z)))
    torch.cuda.synchronize()
    assert_planes(result(d_true, d_status, d_steps, d_column, st), host, "planes")
    assert z.value == host.zenith_column
    d_body, d_rgb = image_planes()
    torch.cuda.synchronize()
    gpu_ctx.check(lib.atmrt_sky_shade_planes_device(gpu_ctx.handle, C.byref(shade), arr, nb, n, d_az.data_ptr(), d_true.data_ptr(), d_status.data_ptr(),
                                                    d_column.data_ptr(), d_body.data_ptr(), d_rgb.data_ptr()))
    torch.cuda.synchronize()
    shade_result(d_body, d_rgb, "shade planes")
    # a reference altitude and a node spacing of the caller's: only Z0 changes
    other = generators.sky_light(gpu_ctx, W, H, ref_alt=2500.0, column_dz=250.0, **SPEC)
    assert_planes(other, host, "other reference")
    assert 0.7 * host.zenith_column < other.zenith_column < 0.78 * host.zenith_column


def test_the_lifted_sun(gpu_ctx, oracle_det):
    """The sun of tests/sky_cases.py whose whole disc lies below the astronomical horizon, shaded: the device equals the model, its
    disc is red (R >= G >= B, R > B) and the sky beside it white.  Then the discs at a sky step of 100 m and of 1000 m side by side: a
    record of what the cheap step costs the colours, nothing asserted."""
    cfg, tiles = lc.lifted_frame()
    res = run_gpu(gpu_ctx, cfg, tiles)
    W, H = res["width"], res["height"]
    setting = slm.Setting.of_config(oracle_det, cfg)
    want = slm.frame(setting, res, lc.LIFTED_H0, lc.STEP, lc.TOP, lc.FLOOR, lc.M)
    z0 = slm.zenith_column(setting, lc.REF_ALT, lc.TOP, lc.STEP)
    assert want.stats["exit"] == W * H  # all sky, on the model first
    plain = np.zeros((H, W, 3), dtype=np.uint8)
    want_body, want_image = slm.shade(plain, z0, [lc.LIFTED_SUN], res["azimuth"], want.true_elevation, want.status, want.column)
    light = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, **SPEC)
    assert_planes(light, want, "lifted")
    image = plain.copy()
    body = generators.sky_shade(gpu_ctx, light, [lc.LIFTED_SUN], image)
    disc = body == 1
    print(f"sky light lifted sun: {int(disc.sum())} disc pixels, air mass {light.air_mass[disc].min():.2f} .. {light.air_mass[disc].max():.2f}, "
          f"colours {image[disc].min(axis=0).tolist()} .. {image[disc].max(axis=0).tolist()}")
    assert body.tobytes() == want_body.tobytes() and image.tobytes() == want_image.tobytes()
    r, g, b = (image[disc][:, c].astype(int) for c in range(3))
    assert disc.sum() > 0 and (r >= g).all() and (g >= b).all() and (r > b).all() and (image[~disc] == 255).all()
    fine = generators.sky_light(gpu_ctx, W, H, ref_alt=lc.REF_ALT, column_dz=lc.STEP, step=100.0, top=lc.TOP, floor=lc.FLOOR, m=15 * lc.M)
    image_fine = plain.copy()
    body_fine = generators.sky_shade(gpu_ctx, fine, [lc.LIFTED_SUN], image_fine)
    rel = np.abs(fine.column / light.column - 1.0)
    print(f"sky light step 100 m | 1000 m: {int((body_fine != body).sum())} of {W * H} body pixels differ, {int((image_fine != image).any(axis=2).sum())} pixels differ in "
          f"colour by at most {int(np.abs(image_fine.astype(int) - image.astype(int)).max())}, largest relative column difference {rel.max():.3g}")
    for a, b2 in zip(image_fine[:, :, 0], image[:, :, 0]):
        print("".join(" .:-=+*#%@"[min(9, int(v) // 5)] if v < 255 else " " for v in a), "|", "".join(" .:-=+*#%@"[min(9, int(v) // 5)] if v < 255 else " " for v in b2))


def test_refusals_that_need_a_context(gpu_ctx, frames):
    cfg, res, _, z0 = frames(gpu_ctx, "rect")
    W, H = res["width"], res["height"]
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    bad, state = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_STATE
    true, column = np.zeros((H, W)), np.zeros((H, W))
    status, steps, body = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint32), np.zeros((H, W), dtype=np.uint8)
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    e, rec, col4 = np.zeros(4), np.zeros(4, dtype=generators.SKY_RAY_DTYPE), np.zeros(4)
    one = (_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0))
    good_sky = generators.sky_spec(**SPEC)
    good_shade = generators.sky_shade_params(z0)

    def light_call(handle, spec, true_p=true.ctypes.data, status_p=status.ctypes.data, column_p=column.ctypes.data):
        return lib.atmrt_sky_light(handle, None if spec is None else C.byref(spec), true_p, status_p, steps.ctypes.data, column_p, None, None)

    def shade_call(handle, shade=good_shade, bodies=one, nb=1, column_p=column.ctypes.data, body_p=body.ctypes.data, rgb_p=rgb.ctypes.data):
        return lib.atmrt_sky_shade(handle, None if shade is None else C.byref(shade), bodies, nb, true.ctypes.data, status.ctypes.data, column_p, body_p, rgb_p)

    assert light_call(h, generators.sky_light_spec(0.0, sky=good_sky)) == 0 and shade_call(h) == 0
    assert lib.atmrt_sky_light_rays(h, C.byref(good_sky), 1000.0, 4, e.ctypes.data, rec.ctypes.data, col4.ctypes.data, None) == 0
    for step, top, floor, m in ((-1.0, 1e5, 0.0, 1500), (math.nan, 1e5, 0.0, 1500), (1000.0, math.inf, 0.0, 1500), (1000.0, 1e5, 1e5, 1500),
                                (1000.0, 1e5, 0.0, 0), (1000.0, 1e5, 0.0, 1048576)):
        sky = generators.sky_spec(step, top, floor, m)
        assert light_call(h, generators.sky_light_spec(0.0, sky=sky)) == bad, (step, top, floor, m)
        assert lib.atmrt_sky_light_rays(h, C.byref(sky), 1000.0, 4, e.ctypes.data, rec.ctypes.data, col4.ctypes.data, None) == bad
    for ref_alt, dz in ((math.nan, 0.0), (math.inf, 0.0), (1e5, 0.0), (2e5, 0.0), (0.0, -1.0), (0.0, math.nan), (0.0, math.inf), (0.0, 0.09)):
        assert light_call(h, generators.sky_light_spec(ref_alt, dz, sky=good_sky)) == bad, (ref_alt, dz)
    assert b"1048575 nodes" in lib.atmrt_last_error(h)
    assert light_call(h, None) == bad and light_call(h, generators.sky_light_spec(0.0, sky=good_sky), true_p=None) == bad
    assert light_call(h, generators.sky_light_spec(0.0, sky=good_sky), status_p=None) == bad and light_call(h, generators.sky_light_spec(0.0, sky=good_sky), column_p=None) == bad
    assert lib.atmrt_sky_light_rays(h, C.byref(good_sky), 1000.0, 4, e.ctypes.data, rec.ctypes.data, None, None) == bad
    assert lib.atmrt_sky_light_rays(h, C.byref(good_sky), math.nan, 4, e.ctypes.data, rec.ctypes.data, col4.ctypes.data, None) == bad
    assert shade_call(h, shade=None) == bad and shade_call(h, bodies=None) == bad and shade_call(h, column_p=None) == bad
    assert shade_call(h, body_p=None) == bad and shade_call(h, rgb_p=None) == bad
    assert shade_call(h, bodies=(_abi.SkyBody * 33)(*[generators.sky_body(100.0, 3.0)] * 33), nb=33) == bad
    assert shade_call(h, bodies=(_abi.SkyBody * 1)(generators.sky_body(100.0, 3.0, 90.0))) == bad
    for kw in (dict(zenith_column=0.0), dict(zenith_column=math.nan), dict(tau=(0.1, -0.1, 0.1)), dict(limb=(0.5, 1.5, 0.5)), dict(exposure=-1.0), dict(exposure=math.inf)):
        args = dict(zenith_column=z0)
        args.update(kw)
        assert shade_call(h, shade=generators.sky_shade_params(**args)) == bad, kw
    assert lib.atmrt_last_sky_shade_timing(h, None) == bad
    # step 0 takes the context's simulation_step, column_dz 0 the step of the march
    rec0, col0, _ = generators.sky_light_rays(gpu_ctx, 1000.0, [0.0, 5.0], step=0.0, top=lc.TOP, floor=lc.FLOOR, m=20000)
    rec1, col1, _ = generators.sky_light_rays(gpu_ctx, 1000.0, [0.0, 5.0], step=cfg.params.simulation_step, top=lc.TOP, floor=lc.FLOOR, m=20000)
    assert rec0.tobytes() == rec1.tobytes() and col0.tobytes() == col1.tobytes() and (rec0["status"] == slm.EXIT).all() and (col0 > 0.0).all()
    a = generators.sky_light(gpu_ctx, W, H, column_dz=0.0, **SPEC).zenith_column
    assert a == generators.sky_light(gpu_ctx, W, H, column_dz=lc.STEP, **SPEC).zenith_column == z0
    # no parameters, then parameters and no frame
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert light_call(fresh.handle, generators.sky_light_spec(0.0, sky=good_sky)) == state and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, fresh))._configure()
        assert light_call(fresh.handle, generators.sky_light_spec(0.0, sky=good_sky)) == state and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert shade_call(fresh.handle) == state
        assert lib.atmrt_sky_light_rays(fresh.handle, C.byref(good_sky), 1000.0, 4, e.ctypes.data, rec.ctypes.data, col4.ctypes.data, None) == 0
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles({}, multi))._configure()
        assert light_call(multi.handle, generators.sky_light_spec(0.0, sky=good_sky)) == state
        assert b"atmrt_sky_light_planes_device" in lib.atmrt_last_error(multi.handle)
        assert shade_call(multi.handle) == state
    finally:
        multi.close()


def test_gen_sky_colour(gpu_ctx, tmp_path):
    """`gen --sun ... --sky-colour --sky-out` end to end: the npz holds the planes of the library's call for the same configuration,
    the image is the shaded one, and without --sky-colour the outputs are those of before."""
    import yaml
    from PIL import Image
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    W, H = 96, 48
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": 2500.0}},
                    "frame": {"direction": 0.0, "fov": 8.0, "tilt": 0.0, "max_distance": 60000.0},
                    "coloring": {"Simple": {"water_level": 300.0, "max_distance": 60000.0}}},
           "simulation_step": 100.0, "output": {"width": W, "height": H, "generator": "Rectilinear"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))

    def gen(out, *extra):
        r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", out, *extra], cwd=str(tmp_path),
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(tmp_path / out).convert("RGB")), r.stdout

    flat, _ = gen("flat.png", "--sun", "1.0", "0.8", "--sky-step", "1000", "--sky-out", "flat.npz")
    shaded, text = gen("shaded.png", "--sun", "1.0", "0.8", "--sky-step", "1000", "--sky-out", "sky.npz", "--sky-colour", "--sky-exposure", "3",
                       "--air-mass-ref", "2500")
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain).generate()
    light = generators.sky_light(gpu_ctx, W, H, step=1000.0, ref_alt=2500.0)
    sun = generators.sky_body(1.0, 0.8, generators.SUN_RADIUS_DEG, (255, 244, 214))
    data, old = np.load(tmp_path / "sky.npz"), np.load(tmp_path / "flat.npz")
    print(f"sky light cli: {light.stats}, Z0 {light.zenith_column!r}; {text.splitlines()[-4:]}")
    assert set(old.files) == {"true_elevation", "status", "steps", "body"} | {"stats_" + k for k in light.stats}  # as before the feature
    assert set(data.files) == set(old.files) | {"column", "air_mass", "zenith_column"}
    for k in ("true_elevation", "status", "steps", "body"):
        assert bits(data[k]).tobytes() == bits(old[k]).tobytes(), k
    assert bits(data["true_elevation"]).tobytes() == bits(light.true_elevation).tobytes() and data["status"].tobytes() == light.status.tobytes()
    assert bits(data["column"]).tobytes() == bits(light.column).tobytes() and float(data["zenith_column"]) == light.zenith_column
    assert bits(data["air_mass"]).tobytes() == bits(light.air_mass).tobytes()
    exits = light.status == slm.EXIT
    differ = (shaded != flat).any(axis=2)
    assert differ.sum() >= 1 and not differ[~exits].any()  # terrain, ticks and lines are those of the flat image
    # the shaded image's sky is the library's shade over the flat image's (the overlay's pixels aside: compared where nothing is drawn)
    image = flat.copy()
    body = generators.sky_shade(gpu_ctx, light, [sun], image, exposure=3.0)
    assert body.tobytes() == data["body"].tobytes() and 0 < (body != 0).sum() < W * H
    same = (image == shaded).all(axis=2)
    assert same[exits].mean() > 0.9 and same[body != 0].any()
