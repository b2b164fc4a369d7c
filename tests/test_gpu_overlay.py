"""atmrt_draw_overlay* on the GPU against tests/overlay_model.py, byte for byte over the whole RGB image: got = draw_image then the
library's overlay, want = the model applied to the same draw_image output and the frame's own azimuth / elevation planes.

Steep segments.  In a roll-free pinhole image (Rectilinear, InterpolatingRectilinear: rectilinear.rs:78-100) the rows of elevation
0 are ONE image row — dir_vec.z = 0 does not depend on x — and a line of constant elevation e is a hyperbola of slope at most
sin e / cos tilt (0.024 rows per column at the flat horizon's 1.3 degrees and tilt -20); a Fast frame's elevation does not depend
on the column at all.  So no frame of the three generators joins two columns more than one row apart (measured on the frames
below: `steepest` is 0 or 1, printed by the tests), and the interior of the line rule, which only matters from |dy| = 2 on, is
exercised where such segments do exist: explicit planes of a rolled camera through atmrt_draw_overlay_planes_device
(test_steep_segments_on_the_planes_of_a_rolled_camera asserts that the model drew them)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import overlay_model as om
from atm_raytracer_amd import _abi, config, generators, synth
from util import run_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README_TICKS = [("Multiple", 0.0, 10.0, 10, True), ("Multiple", 0.0, 2.0, 5, False), ("Single", 45.0, 15, True)]
VTICKS = [("Multiple", 0.0, 5.0, 8, True), ("Multiple", 0.5, 1.0, 3, False), ("Single", -2.25, 12, True)]


def scene(generator, w, h, **over):
    over.setdefault("max_distance", 60_000.0)
    cfg, tiles = synth.scene("S2", w, h, generator=generator, **over)
    cfg.coloring = config._coloring({})
    return cfg, tiles


def frame_of(p):
    return {"direction": p.frame.direction, "fov": p.frame.fov, "tilt": p.frame.tilt, "width": p.width, "height": p.height}


def overlay_of(ticks, vticks, eye, flat):
    return generators.into_overlay({"ticks": ticks, "vertical_ticks": vticks, "show_eye_level": eye, "show_flat_horizon": flat})


def expected_flat_horizon(ctx, cfg):
    """degrees(acos(1 / n)) with n from atmrt_atmosphere_sample at the observer's absolute altitude (params.rs:23-30), or None when
    the condition of renderer/mod.rs:420-422 does not hold (the caller has checked show_flat_horizon)."""
    p = cfg.params
    flat = p.earth.kind in (_abi.EARTH_KINDS["AzimuthalEquidistant"], _abi.EARTH_KINDS["FlatDistorted"], _abi.EARTH_KINDS["ObserverAe"],
                            _abi.EARTH_KINDS["SimpleObserverAe"])
    if not flat or p.straight_rays:
        return None
    alt = p.position.altitude
    if p.position.altitude_kind == _abi.ALT_RELATIVE:
        elev, valid = generators.Terrain(ctx).get_elev(p.position.latitude, p.position.longitude)
        alt = (float(elev[0]) if valid[0] else 0.0) + p.position.altitude
    n = float(generators.atmosphere_sample(ctx, [alt])["n"][0])
    return math.degrees(math.acos(1.0 / n))


def run_case(ctx, cfg, tiles, ticks, vticks, eye, flat):
    """-> (got image, want image, got ticks, model info, flat_horizon_deg, base image)."""
    res = run_gpu(ctx, cfg, tiles)
    h, w = res["hit_count"].shape
    col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
    base = generators.draw_image(ctx, col, w, h)
    got, got_ticks, deg = generators.draw_overlay(ctx, overlay_of(ticks, vticks, eye, flat), base)
    target = expected_flat_horizon(ctx, cfg) if flat else None
    want, want_ticks, info = om.draw_overlay(base, frame_of(cfg.params), ticks, vticks, eye, target, res["azimuth"], res["elevation_angle"])
    print(f"{cfg.params.generator=} {w}x{h} tilt={cfg.params.frame.tilt} ticks={len(got_ticks)} flat_deg={deg!r} steepest={info['steepest']} "
          f"eye_found={None if info['eye_y'] is None else sum(y is not None for y in info['eye_y'])}")
    assert got_ticks == want_ticks
    if target is None:
        assert math.isnan(deg)
    else:
        assert deg == target  # bit for bit
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    return got, want, got_ticks, info, deg, base


CASES = {
    "fast": dict(generator="Fast", w=96, h=48, over=dict(tilt=-3.0)),
    "fast-wide": dict(generator="Fast", w=512, h=256, over=dict(tilt=-3.0)),  # many columns, several row bands
    "rect-tilt3": dict(generator="Rectilinear", w=96, h=48, over=dict(tilt=-3.0)),
    "rect-tilt20-fov90": dict(generator="Rectilinear", w=96, h=64, over=dict(tilt=-20.0, fov=90.0)),
    "interp": dict(generator="InterpolatingRectilinear", w=96, h=48, over=dict(tilt=-3.0)),
}


@pytest.mark.parametrize("earth", ["Spherical", "FlatDistorted"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_overlay_matches_the_model(gpu_ctx, name, earth):
    c = CASES[name]
    over = dict(c["over"])
    if earth == "FlatDistorted":
        over["earth_shape"] = "FlatDistorted"
    cfg, tiles = scene(c["generator"], c["w"], c["h"], **over)
    got, want, ticks, info, deg, base = run_case(gpu_ctx, cfg, tiles, README_TICKS, VTICKS, True, True)
    assert ticks and (got != base).any()
    assert sum(y is not None for y in info["eye_y"]) >= c["w"] // 2  # the eye-level line is in view
    if earth == "FlatDistorted":
        assert 0.5 < deg < 2.5 and info["flat_y"] is not None and sum(y is not None for y in info["flat_y"]) >= c["w"] // 2
        assert (got == om.FLAT_HORIZON_COLOR).all(axis=2).sum() >= c["w"] // 2
    else:
        assert math.isnan(deg) and not (got == om.FLAT_HORIZON_COLOR).all(axis=2).any()


def test_straight_rays_draw_no_flat_horizon(gpu_ctx):
    cfg, tiles = scene("Fast", 96, 48, tilt=-3.0, earth_shape="FlatDistorted", straight_rays=True)
    got, _, _, info, deg, _ = run_case(gpu_ctx, cfg, tiles, [], [], True, True)
    assert math.isnan(deg) and info["flat_y"] is None and not (got == om.FLAT_HORIZON_COLOR).all(axis=2).any()


def test_eye_level_out_of_view_leaves_the_image_alone(gpu_ctx):
    cfg, tiles = scene("Fast", 96, 48, tilt=-30.0, fov=20.0)
    got, _, ticks, info, _, base = run_case(gpu_ctx, cfg, tiles, [], [], True, True)
    assert info["eye_y"] == [None] * 96 and ticks == [] and np.array_equal(got, base)


def test_layer_order_where_tick_and_both_lines_cross(gpu_ctx):
    """FlatDistorted, tilt 0: a vertical tick at the flat horizon's elevation, longer than half the width, lies under the
    flat-horizon line; one at elevation 0 under the eye-level line; the horizontal tick of the centre column crosses both."""
    w, h = 96, 48
    cfg, tiles = scene("Fast", w, h, tilt=0.0, earth_shape="FlatDistorted")
    run_gpu(gpu_ctx, cfg, tiles)
    target = expected_flat_horizon(gpu_ctx, cfg)
    vt = [("Single", 0.0, 60, False), ("Single", target, 60, False)]
    got, want, ticks, info, deg, base = run_case(gpu_ctx, cfg, tiles, [("Single", 0.0, 40, False)], vt, True, True)
    y_eye, y_flat = info["eye_y"][0], info["flat_y"][0]
    assert y_eye is not None and y_flat is not None and y_flat < y_eye and len(ticks) == 3
    assert (got[y_eye, :] == om.EYE_LEVEL_COLOR).all() and (got[y_flat, :] == om.FLAT_HORIZON_COLOR).all()
    x = [t for t in ticks if not t["vertical"]][0]["pos"]
    assert (got[0, x] == om.WHITE).all() and (got[40, x] == om.WHITE).all() and (base[y_eye, x] != om.EYE_LEVEL_COLOR).any()


def test_column_shard_is_an_image_of_its_own(gpu_ctx):
    """col_begin / col_end: the overlay runs on the shard's planes; the ranges of Multiple ticks still come from the frame."""
    cfg, tiles = scene("Fast", 128, 48, tilt=-2.0, earth_shape="FlatDistorted")
    cfg.params.col_begin, cfg.params.col_end = 37, 101
    got, want, ticks, info, _, _ = run_case(gpu_ctx, cfg, tiles, README_TICKS, VTICKS, True, True)
    assert got.shape == (48, 64, 3) and ticks and all(t["pos"] < 64 for t in ticks if not t["vertical"])


def rolled_planes(w, h):
    """A camera rolled so that the horizon climbs 3.3 rows per column towards both edges (a V), with a hole of NaN."""
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    el = (h * 0.2 + 3.3 * np.abs(x - w / 2.0 + 0.25) - y) * 0.1
    el[h // 3: h // 3 + 2, w // 4] = np.nan
    az = np.broadcast_to(10.0 + (x - w / 2.0) * 0.25, (h, w)).copy()
    return az, el


def test_steep_segments_on_the_planes_of_a_rolled_camera(gpu_ctx):
    """The interior of the line rule (segments with |dy| >= 2, both directions) through atmrt_draw_overlay_planes_device."""
    w, h = 80, 160
    cfg, tiles = scene("Fast", w, h, direction=10.0, fov=20.0, earth_shape="FlatDistorted")
    run_gpu(gpu_ctx, cfg, tiles)  # the context's frame: position and atmosphere of the flat horizon
    target = expected_flat_horizon(gpu_ctx, cfg)
    az, el = rolled_planes(w, h)
    dev = torch.device("cuda", 0)
    base = np.random.default_rng(3).integers(0, 200, size=(h, w, 3), dtype=np.uint8)
    t_az, t_el, t_rgb = torch.from_numpy(az).to(dev), torch.from_numpy(el).to(dev), torch.from_numpy(base).to(dev)
    ticks, deg = generators.draw_overlay_device(gpu_ctx, overlay_of(README_TICKS, VTICKS, True, True), t_rgb.data_ptr(), w, h,
                                                planes=(t_az.data_ptr(), t_el.data_ptr()))
    want, want_ticks, info = om.draw_overlay(base, frame_of(cfg.params), README_TICKS, VTICKS, True, target, az, el)
    ys = [y for y in info["eye_y"] if y is not None]
    steps = [b - a for a, b in zip(info["eye_y"], info["eye_y"][1:]) if a is not None and b is not None]
    print(f"steepest={info['steepest']} found={len(ys)} steps={sorted(set(steps))}")
    assert info["steepest"] >= 3 and min(steps) <= -2 and max(steps) >= 2  # the model drew steep segments in both directions
    assert deg == target and ticks == want_ticks
    assert np.array_equal(t_rgb.cpu().numpy(), want)


def test_state_and_argument_errors(gpu_ctx):
    lib = gpu_ctx.lib
    o = overlay_of([], [], True, True)
    rgb = np.zeros((48, 96, 3), dtype=np.uint8)
    call = lambda c: lib.atmrt_draw_overlay(c.handle, C.byref(o), rgb.ctypes.data, None, 0, None, None)
    fresh = generators.Context(0)
    try:
        assert call(fresh) == _abi.ERR_STATE and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        dev_rgb = torch.zeros((48, 96, 3), dtype=torch.uint8, device="cuda")
        assert lib.atmrt_draw_overlay_device(fresh.handle, C.byref(o), dev_rgb.data_ptr(), None, 0, None, None) == _abi.ERR_STATE
        cfg, tiles = scene("Fast", 96, 48)
        run_gpu(fresh, cfg, tiles)
        assert call(fresh) == 0
        assert lib.atmrt_draw_overlay(fresh.handle, None, rgb.ctypes.data, None, 0, None, None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.atmrt_draw_overlay(fresh.handle, C.byref(o), None, None, 0, None, None) == _abi.ERR_INVALID_ARGUMENT
        bad = overlay_of([("Multiple", 0.0, 0.0, 3, True)], [], False, False)
        assert lib.atmrt_draw_overlay(fresh.handle, C.byref(bad), rgb.ctypes.data, None, 0, None, None) == _abi.ERR_INVALID_ARGUMENT
        many = overlay_of(README_TICKS, [], False, False)
        rgb[:] = 0
        arr, n = (_abi.DrawnTick * 1)(), C.c_size_t()
        assert lib.atmrt_draw_overlay(fresh.handle, C.byref(many), rgb.ctypes.data, arr, 1, C.byref(n), None) == _abi.ERR_INVALID_ARGUMENT
        assert n.value > 1 and not rgb.any()  # refused before anything is drawn
        # after a failed frame the planes of the frame before it are gone
        assert lib.atmrt_debug_fail_next_frame(fresh.handle) == 0
        with pytest.raises(generators.AtmrtError):
            run_gpu(fresh, cfg, tiles)
        assert call(fresh) == _abi.ERR_STATE
        # H = 1 (and W = 1): the reference would index row / column 1
        run_gpu(fresh, cfg, tiles)
        for w1, h1 in ((96, 1), (1, 48)):
            rc = lib.atmrt_draw_overlay_planes_device(fresh.handle, C.byref(o), dev_rgb.data_ptr(), dev_rgb.data_ptr(), w1, h1, dev_rgb.data_ptr(),
                                                      None, 0, None, None)
            assert rc == _abi.ERR_INVALID_ARGUMENT and b"2 x 2" in lib.atmrt_last_error(fresh.handle)
    finally:
        fresh.close()


@pytest.mark.parametrize("n_tiles", [2, 5])
def test_gathered_planes_of_a_multi_device_context(gpu_ctx, n_tiles):
    """atmrt_draw_overlay_planes_device on the gathered [H][W] planes + the gathered RGB image equals the single-context result;
    the last-frame entry points of the parent return ATMRT_ERR_STATE and name it."""
    w, h = (90, 40) if n_tiles == 2 else (93, 40)
    cfg, tiles = scene("Fast", w, h, tilt=-2.0, earth_shape="FlatDistorted")
    single, _, single_ticks, _, single_deg, _ = run_case(gpu_ctx, cfg, tiles, README_TICKS, VTICKS, True, True)
    ctx = generators.Context.multi([0] * n_tiles)
    try:
        gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
        dev = torch.device("cuda", 0)
        images = [generators.image_planes(h, w, dev) for _ in range(n_tiles)]
        gen.generate_image_device([pod for _, pod in images])
        col = generators.into_coloring(ctx.lib, cfg.params, cfg.coloring)
        rgbs = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(n_tiles)]
        ptrs = (C.c_void_p * n_tiles)(*[t.data_ptr() for t in rgbs])
        ctx.check(ctx.lib.atmrt_draw_image_gathered_device(ctx.handle, C.byref(col), ptrs))
        o = overlay_of(README_TICKS, VTICKS, True, True)
        assert ctx.lib.atmrt_draw_overlay_device(ctx.handle, C.byref(o), rgbs[0].data_ptr(), None, 0, None, None) == _abi.ERR_STATE
        assert b"atmrt_draw_overlay_planes_device" in ctx.lib.atmrt_last_error(ctx.handle)
        host = np.zeros((h, w, 3), dtype=np.uint8)
        assert ctx.lib.atmrt_draw_overlay(ctx.handle, C.byref(o), host.ctypes.data, None, 0, None, None) == _abi.ERR_STATE
        planes = images[-1][0]
        ticks, deg = generators.draw_overlay_device(ctx, o, rgbs[-1].data_ptr(), w, h,
                                                    planes=(planes["azimuth"].data_ptr(), planes["elevation_angle"].data_ptr()))
        assert ticks == single_ticks and deg == single_deg
        assert np.array_equal(rgbs[-1].cpu().numpy(), single)
    finally:
        ctx.close()


def test_cli_gen_draws_ticks_lines_and_labels(tmp_path):
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 40.0, "fov": 30.0, "tilt": -2.0, "max_distance": 60000.0}},
           "simulation_step": 100.0, "output": {"width": 240, "height": 120, "generator": "Fast"}}
    (tmp_path / "plain.yaml").write_text(yaml.safe_dump(doc))
    doc["output"].update({"ticks": [{"Multiple": {"bias": 0, "step": 10, "size": 10, "labelled": True}},
                                    {"Multiple": {"bias": 0, "step": 2, "size": 5, "labelled": False}},
                                    {"Single": {"azimuth": 45, "size": 15, "labelled": True}}],
                          "show_eye_level": True, "show_flat_horizon": False})
    (tmp_path / "ticks.yaml").write_text(yaml.safe_dump(doc))
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = {}
    for name in ("plain", "ticks"):
        r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", f"{name}.yaml", "--output", f"{name}.png", "--metadata",
                            f"{name}.npz"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[name] = r
    from PIL import Image
    plain, got = (np.asarray(Image.open(tmp_path / f"{n}.png")) for n in ("plain", "ticks"))
    assert (plain != got).any()
    meta = np.load(tmp_path / "ticks.npz")
    cfg = config.parse_config(str(tmp_path / "ticks.yaml"))
    want, ticks, info = om.draw_overlay(plain, frame_of(cfg.params), cfg.output["ticks"], [], True, None, meta["azimuth"], meta["elevation_angle"])
    labelled = [t for t in ticks if t["labelled"]]
    assert {t["label"] for t in labelled} == {"30", "40", "50", "45"} and sum(y is not None for y in info["eye_y"]) == 240
    mask = np.zeros(got.shape[:2], dtype=bool)  # the label boxes: anchored at (x - 8, size + 5), 15 px high
    for t in labelled:
        mask[t["size"] + 5: t["size"] + 5 + 16, max(0, t["pos"] - 8): t["pos"] - 8 + 10 * len(t["label"])] = True
    assert np.array_equal(got[~mask], want[~mask])
    from atm_raytracer_amd.__main__ import find_label_font
    if find_label_font() is None:
        assert "tick labels are left off" in outs["ticks"].stderr and np.array_equal(got, want)
    else:
        assert (got[mask] != want[mask]).any()  # glyph pixels inside the boxes
