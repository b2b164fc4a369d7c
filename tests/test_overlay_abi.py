"""The host half of the overlay entry points (include/atmrt.h: atmrt_overlay_resolve_ticks, the struct sizes, the Python mirrors)
against tests/overlay_model.py.  The library loads without a GPU; nothing here touches a device."""
import ctypes as C
import math

import numpy as np
import pytest
import yaml

import overlay_model as om
from atm_raytracer_amd import _abi, _lib, config, generators

# the tick block of the reference README's example config (README.md:238-272), as the YAML a user writes
README_OUTPUT = """
output:
    width: 960
    height: 600
    ticks:
      - Multiple: {bias: 0, step: 10, size: 10, labelled: true}
      - Multiple: {bias: 0, step: 2, size: 5, labelled: false}
      - Single: {azimuth: 45, size: 15, labelled: true}
    show_eye_level: true
    show_flat_horizon: false
    generator: Fast
"""
README_TICKS = [("Multiple", 0.0, 10.0, 10, True), ("Multiple", 0.0, 2.0, 5, False), ("Single", 45.0, 15, True)]


@pytest.fixture(scope="module")
def lib():
    if not _lib.os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def overlay_of(ticks, vertical_ticks, eye=False, flat=False):
    return generators.into_overlay({"ticks": ticks, "vertical_ticks": vertical_ticks, "show_eye_level": eye, "show_flat_horizon": flat})


def params_of(direction, fov, tilt, w, h, col_begin=0, col_end=0):
    p = _abi.Params()
    _lib.load().atmrt_params_default(C.byref(p))
    p.frame.direction, p.frame.fov, p.frame.tilt = direction, fov, tilt
    p.width, p.height, p.col_begin, p.col_end = w, h, col_begin, col_end
    return p


def frame_of(p):
    return {"direction": p.frame.direction, "fov": p.frame.fov, "tilt": p.frame.tilt, "width": p.width, "height": p.height}


def fast_rows(direction, fov, tilt, w, h):
    """Fast-style: linear in the pixel index, azimuth wrapped once into [0, 360) (fast.rs:67-72)."""
    az = direction + (np.arange(w) - w / 2.0) * fov / w
    az = np.where(az < 0.0, az + 360.0, np.where(az >= 360.0, az - 360.0, az))
    el = tilt - (np.arange(h) - h / 2.0) * fov / w
    return az, el


def pinhole_rows(direction, fov, tilt, w, h):
    """Pinhole-style: the tangent plane of a rectilinear lens, azimuth left unwrapped around the direction in (-180, 180]."""
    d = direction - 360.0 if direction > 180.0 else direction
    t = math.tan(math.radians(fov / 2.0)) / (w / 2.0)
    az = d + np.degrees(np.arctan((np.arange(w) - w / 2.0 + 0.5) * t))
    el = tilt - np.degrees(np.arctan((np.arange(h) - h / 2.0 + 0.5) * t))
    return az, el


def model_ticks(p, ticks, vticks, az, el):
    hor, ver = om.gen_ticks(frame_of(p), ticks, vticks, az.reshape(1, -1), el.reshape(-1, 1))
    return om.ticks_sorted(hor, ver)


def test_struct_sizes_match_the_header(lib):
    for which, st in ((14, _abi.Tick), (15, _abi.Overlay), (16, _abi.DrawnTick)):
        assert lib.atmrt_abi_sizeof(which) == C.sizeof(st), st.__name__
    assert lib.atmrt_abi_sizeof(17) == 0 and lib.atmrt_abi_version() == 5
    assert C.sizeof(_abi.DrawnTick) == 16 + _abi.TICK_LABEL_BYTES
    for name in ("atmrt_overlay_resolve_ticks", "atmrt_draw_overlay_device", "atmrt_draw_overlay", "atmrt_draw_overlay_planes_device"):
        assert name in _lib.EXPORTED and hasattr(lib, name)


def test_into_overlay_of_the_readme_example():
    cfg = config.Config.from_dict(yaml.safe_load(README_OUTPUT))
    assert cfg.output["ticks"] == README_TICKS and cfg.output["vertical_ticks"] == []
    o = generators.into_overlay(cfg.output)
    assert (o.n_ticks, o.n_vertical_ticks, o.show_eye_level, o.show_flat_horizon) == (3, 0, 1, 0)
    got = [(t.kind, t.size, t.angle, t.bias, t.step, t.labelled) for t in (o.ticks[i] for i in range(3))]
    assert got == [(_abi.TICK_MULTIPLE, 10, 0.0, 0.0, 10.0, 1), (_abi.TICK_MULTIPLE, 5, 0.0, 0.0, 2.0, 0), (_abi.TICK_SINGLE, 15, 45.0, 0.0, 0.0, 1)]
    cfg = config.Config.from_dict({"output": {"vertical_ticks": [{"Single": {"elevation": -1.5, "size": 4, "labelled": False}}],
                                              "show_flat_horizon": True}})
    o = generators.into_overlay(cfg.output)
    assert (o.n_ticks, o.n_vertical_ticks, o.show_eye_level, o.show_flat_horizon) == (0, 1, 0, 1)
    assert (o.vertical_ticks[0].kind, o.vertical_ticks[0].angle, o.vertical_ticks[0].size) == (_abi.TICK_SINGLE, -1.5, 4)


def test_resolve_ticks_of_the_readme_example(lib):
    """960 x 600, looking at 40 degrees with a 30 degree field: a labelled tick every 10 degrees, a short one every 2, 45 marked."""
    p = params_of(40.0, 30.0, 0.0, 960, 600)
    az, el = fast_rows(40.0, 30.0, 0.0, 960, 600)
    got = generators.resolve_ticks(p, overlay_of(README_TICKS, []), az, el, lib)
    assert got == model_ticks(p, README_TICKS, [], az, el)
    by_pos = {t["pos"]: t for t in got}
    assert by_pos[480] == {"pos": 480, "size": 10, "labelled": True, "vertical": False, "label": "40"}
    assert by_pos[640]["label"] == "45" and by_pos[640]["size"] == 15 and by_pos[544]["size"] == 5 and not by_pos[544]["labelled"]
    assert len(got) == 16  # 25 .. 54 in steps of 2 is 15 ticks, + 45


def random_ticks(rng, vertical, lo, hi):
    out = []
    for _ in range(int(rng.integers(0, 4))):
        labelled = bool(rng.integers(0, 2))
        size = int(rng.integers(1, 40))
        if rng.integers(0, 2):
            angle = float(rng.choice([round(float(rng.uniform(lo - 3, hi + 3)), int(rng.integers(0, 4))), float(rng.uniform(lo, hi))]))
            if not vertical and rng.integers(0, 3) == 0:
                angle += 360.0 * int(rng.integers(-1, 2))
            out.append(("Single", angle, size, labelled))
        else:
            step = float(rng.choice([0.5, 1.0, 2.0, 2.5, 5.0, 10.0, 0.25, 1.0 / 3.0, float(rng.uniform(0.3, 7.0))]))
            bias = float(rng.choice([0.0, 0.0, 1.5, -0.25, float(rng.uniform(-5, 5))]))
            out.append(("Multiple", bias, step, size, labelled))
    return out


def test_resolve_ticks_equals_the_model_over_a_seeded_sweep(lib):
    rng = np.random.default_rng(20240611)
    n_ticks = n_frames = n_labels_with_decimals = 0
    for case in range(120):
        w, h = int(rng.integers(2, 400)), int(rng.integers(2, 240))
        direction = float(rng.choice([0.0, 355.0, 3.0, 180.0, float(rng.uniform(0, 360))]))
        fov = float(rng.uniform(2.0, 100.0))
        tilt = float(rng.choice([0.0, -3.0, -20.0, 85.0, -88.0, float(rng.uniform(-30, 30))]))
        p = params_of(direction, fov, tilt, w, h)
        rows = (fast_rows, pinhole_rows)[case % 2]
        az, el = rows(direction, fov, tilt, w, h)
        if case % 7 == 3 and w >= 8:  # a column shard: the row is the shard's, the ranges stay the frame's
            c0, c1 = sorted(rng.choice(np.arange(w + 1), 2, replace=False))
            if c1 - c0 >= 2:
                p.col_begin, p.col_end = int(c0), int(c1)
                az = az[c0:c1]
        aspect = h / w
        ticks = random_ticks(rng, False, direction - fov / 2, direction + fov / 2)
        vticks = random_ticks(rng, True, tilt - fov * aspect / 2, tilt + fov * aspect / 2)
        if case % 5 == 0:
            ticks = README_TICKS + ticks
        got = generators.resolve_ticks(p, overlay_of(ticks, vticks), az, el, lib)
        want = model_ticks(p, ticks, vticks, az, el)
        assert got == want, (case, w, h, direction, fov, tilt, ticks, vticks)
        n_ticks += len(got)
        n_frames += bool(got)
        n_labels_with_decimals += sum("." in t["label"] for t in got)
    assert n_frames > 60 and n_ticks > 1000 and n_labels_with_decimals > 100, (n_frames, n_ticks, n_labels_with_decimals)


def test_resolve_ticks_refuses_bad_arguments(lib):
    p = params_of(40.0, 30.0, 0.0, 64, 32)
    az, el = fast_rows(40.0, 30.0, 0.0, 64, 32)
    o = overlay_of(README_TICKS, [("Single", 0.0, 3, True)])
    n = C.c_size_t()
    call = lambda p_, o_, az_, el_, arr, cap, n_: lib.atmrt_overlay_resolve_ticks(p_, o_, az_, el_, arr, cap, n_)
    azp, elp = az.ctypes.data, el.ctypes.data
    assert call(C.byref(p), C.byref(o), azp, elp, None, 0, C.byref(n)) == 0 and n.value == len(model_ticks(p, README_TICKS, [("Single", 0.0, 3, True)], az, el))
    arr = (_abi.DrawnTick * n.value)()
    assert call(C.byref(p), C.byref(o), azp, elp, arr, n.value - 1, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT  # capacity too small
    assert call(C.byref(p), C.byref(o), azp, elp, arr, n.value, C.byref(n)) == 0
    assert call(None, C.byref(o), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert call(C.byref(p), None, azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert call(C.byref(p), C.byref(o), None, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert call(C.byref(p), C.byref(o), azp, None, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert call(C.byref(p), C.byref(o), azp, elp, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    for w, h in ((1, 32), (64, 1), (0, 0)):  # the reference indexes neighbour 1
        assert call(C.byref(params_of(40.0, 30.0, 0.0, w, h)), C.byref(o), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert call(C.byref(params_of(40.0, 30.0, 0.0, 64, 32, 10, 11)), C.byref(o), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    for bad in (("Multiple", 0.0, 0.0, 3, True), ("Multiple", 0.0, -1.0, 3, True), ("Multiple", 0.0, float("nan"), 3, True),
                ("Multiple", 0.0, float("inf"), 3, True), ("Multiple", 0.0, 1e-9, 3, True)):  # the reference would loop (nearly) for ever
        for o_bad in (overlay_of([bad], []), overlay_of([], [bad])):
            assert call(C.byref(p), C.byref(o_bad), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT, bad
    o_kind = overlay_of([("Single", 40.0, 3, True)], [])
    o_kind.ticks[0].kind = 2
    assert call(C.byref(p), C.byref(o_kind), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    o_null = overlay_of([("Single", 40.0, 3, True)], [])
    o_null.ticks = None
    assert call(C.byref(p), C.byref(o_null), azp, elp, None, 0, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    with pytest.raises(_lib.AtmrtError):
        generators.resolve_ticks(p, overlay_of([("Multiple", 0.0, 0.0, 3, True)], []), az, el, lib)
