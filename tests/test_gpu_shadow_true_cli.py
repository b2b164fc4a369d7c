"""`gen --sun AZ EL --shadows --shadow-per-point --shadow-true` end to end on a 48 x 24 frame: the image equals the one drawn from
the status plane of tests/sky_apparent_model.py's solve_true with the sun as the light (and the sun's disc over it); `gen
--shadow-lights FILE.csv --shadow-true` writes the mask of the library's true-direction call; --shadow-true without a light per
point is a configuration error."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

import shadow_lights_model as slm
import shadow_model as sm
import sky_apparent_model as sam
import sky_model as skm
from atm_raytracer_amd import config, generators, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 24
SUN = (300.0, 1.0)  # the sun's TRUE direction: low in the north-west, on the frame's axis (317 points lit, 106 of them by refraction alone)
SUN_RGB = (255, 244, 214)
REACH = 20_000.0
TABLE_ALT, TABLE_EL = (0.0, 3000.0, 3), (-3.0, 9.8, 257)


def write_scene(tmp_path):
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": 2500.0}},
                    "frame": {"direction": 300.0, "fov": 60.0, "tilt": -4.0, "max_distance": 60000.0},
                    "coloring": {"Shading": {"water_level": 300.0, "ambient_light": 0.3, "light_zenith_angle": 88.0, "light_dir": -80.0}}},
           "simulation_step": 100.0, "output": {"width": W, "height": H, "generator": "Rectilinear"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    return tiles


def gen(tmp_path, out, *extra):
    return subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", out, *extra], cwd=str(tmp_path),
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def test_gen_shadow_true_equals_the_model(gpu_ctx, oracle_det, tmp_path):
    tiles = write_scene(tmp_path)
    table_args = ["--sky-step", "1000", "--sky-table-alt", *[repr(v) for v in TABLE_ALT], "--sky-table-el", *[repr(v) for v in TABLE_EL]]
    r = gen(tmp_path, "true.png", "--sun", repr(SUN[0]), repr(SUN[1]), "--shadows", "--shadow-per-point", "--shadow-true", "--shadow-reach", repr(REACH),
            *table_args)
    assert r.returncode == 0, r.stderr
    image = np.asarray(Image.open(tmp_path / "true.png").convert("RGB"))
    g = gen(tmp_path, "geometric.png", "--sun", repr(SUN[0]), repr(SUN[1]), "--shadows", "--shadow-per-point", "--shadow-light", repr(SUN[0]), repr(SUN[1]),
            "--shadow-reach", repr(REACH), "--sky-step", "1000")
    assert g.returncode == 0, g.stderr
    geometric_image = np.asarray(Image.open(tmp_path / "geometric.png").convert("RGB"))
    # the model over the frame the library generates for the same configuration
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    res = generators.make_generator(generators.Params(cfg), terrain).generate()
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        table = sam.build(skm.Setting.of_config(oracle_det, cfg), sam.Spec(TABLE_ALT, TABLE_EL, step=1000.0, top=100000.0, floor=0.0))
        dirs = slm.lights_from_angles(oracle_det, cfg.params, [SUN])
        want = sam.solve_true(setting, table, res, dirs, REACH)
        geometric = slm.solve(setting, res, dirs, REACH)
    finally:
        setting.close()
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, cfg.coloring)
    sun = [generators.sky_body(SUN[0], SUN[1], generators.SUN_RADIUS_DEG, SUN_RGB)]
    sky = generators.sky_directions(gpu_ctx, W, H, steps=False, step=1000.0)
    expected = generators.draw_image(gpu_ctx, coloring, W, H, shadows=want.status[0], bodies=sun, sky=sky)
    expected_geometric = generators.draw_image(gpu_ctx, coloring, W, H, shadows=geometric.status[0], bodies=sun, sky=sky)
    moved = want.status[0] != geometric.status[0]
    lit, dark = int((want.status[0] == sm.LIT).sum()), int((want.status[0] == sm.SHADOWED).sum())
    print(f"gen --shadow-true: {lit} lit, {dark} shadowed, {int(moved.sum())} pixels differ from the geometric rule; {r.stdout.splitlines()[-4:]}")
    assert f"of the world (true direction): {lit} points lit, {dark} in shadow" in r.stdout
    assert image.tobytes() == expected.tobytes(), np.argwhere((image != expected).any(axis=2))[:5]
    assert geometric_image.tobytes() == expected_geometric.tobytes()  # without --shadow-true: what it does today
    assert lit > 0 and dark > 0 and moved.any() and (want.status[0][moved] == sm.LIT).all()  # refraction only lifts the sun
    # the light list under the same rule: the .npz holds the library call's mask and counts
    rows = [SUN, (260.0, 2.0), (225.0, -0.3)]
    (tmp_path / "lights.csv").write_text("azimuth_deg,elevation_deg\n" + "".join(f"{az!r},{el!r}\n" for az, el in rows))
    r = gen(tmp_path, "list.png", "--shadow-lights", "lights.csv", "--shadow-lights-out", "lights.npz", "--shadow-true", "--shadow-reach", repr(REACH), *table_args)
    assert r.returncode == 0, r.stderr
    spec = generators.sky_table_spec(TABLE_ALT, TABLE_EL, step=1000.0)
    listed = generators.shadow_lights(gpu_ctx, generators.lights_from_angles(cfg.params, rows, gpu_ctx.lib), REACH, width=W, height=H, true_table=spec)
    z = np.load(tmp_path / "lights.npz")
    assert z["lit_mask"].tobytes() == listed.lit_mask.tobytes() and {k: int(z["stats_" + k]) for k in listed.stats} == listed.stats
    assert ((listed.lit_mask & np.uint64(1)) != 0).tobytes() == (want.status[0] == sm.LIT).tobytes()  # light 0 is the sun above


def test_shadow_true_needs_a_light_per_point(gpu_ctx, tmp_path):
    write_scene(tmp_path)
    for extra in (["--shadow-true"], ["--shadows", "--shadow-true"], ["--sun", "260", "1", "--shadows", "--shadow-true"]):
        r = gen(tmp_path, "none.png", *extra)
        assert r.returncode == 1 and "--shadow-true needs a light per point" in r.stderr, (extra, r.stderr)
    r = gen(tmp_path, "none.png", "--shadows", "--shadow-per-point", "--shadow-true", "--shadow-light", "260", "1", "--sky-table-el", "5", "1", "9")
    assert r.returncode == 1 and "--sky-table-el" in r.stderr
    assert not os.path.exists(tmp_path / "none.png")
