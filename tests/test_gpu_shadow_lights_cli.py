"""`gen --shadows --shadow-per-point` and `gen --shadow-lights FILE.csv` end to end on a 50 x 20 frame: the image differs from the plain
one exactly at the pixels the Shading configuration's own light_dir vector leaves in shadow and equals there what the library draws
through the Python mirror; the .npz holds the library call's mask, its popcount, the lights and the counts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

from atm_raytracer_amd import _abi, config, generators, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHTS = [(260.0, 2.0), (225.0, 10.0), (180.0, 30.0), (100.0, -1.0), (80.0, 1.5)]


def test_gen_shadow_lights_and_per_point_shadows(gpu_ctx, tmp_path):
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    W, H = 50, 20
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": 2500.0}},
                    "frame": {"direction": 0.0, "fov": 40.0, "tilt": -6.0, "max_distance": 60000.0},
                    "coloring": {"Shading": {"water_level": 300.0, "ambient_light": 0.3, "light_zenith_angle": 88.0, "light_dir": -80.0}}},
           "simulation_step": 100.0, "output": {"width": W, "height": H, "generator": "Rectilinear"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    (tmp_path / "lights.csv").write_text("azimuth_deg,elevation_deg\n# a day's path, shortened\n" + "".join(f"{az!r},{el!r}\n" for az, el in LIGHTS))

    def gen(out, *extra):
        r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", out, *extra], cwd=str(tmp_path),
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(tmp_path / out).convert("RGB")), r.stdout

    plain, _ = gen("plain.png")
    shadowed, text = gen("shadowed.png", "--shadows", "--shadow-per-point", "--shadow-reach", "20000", "--shadow-lights", "lights.csv",
                         "--shadow-lights-out", "lights.npz")
    # the same through the mirror
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain).generate()
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, cfg.coloring)
    one = generators.shadow_lights(gpu_ctx, [list(coloring.light_dir)], 20_000.0, status=True, width=W, height=H)
    want = generators.draw_image(gpu_ctx, coloring, W, H, shadows=one.status[0])
    sh = one.status[0] == _abi.SHADOW_SHADOWED
    differ = (shadowed != plain).any(axis=2)
    print(f"shadow lights cli: {one.stats}, {int(differ.sum())} pixels differ from the plain image; {text.splitlines()[-4:]}")
    assert f"of the world: {one.stats['lit']} points lit, {one.stats['shadowed']} in shadow" in text
    assert differ.sum() >= 1 and not differ[~sh].any()
    assert np.array_equal(shadowed[sh], want[sh])
    # the light list
    dirs = generators.lights_from_angles(cfg.params, LIGHTS, gpu_ctx.lib)
    lights = generators.shadow_lights(gpu_ctx, dirs, 20_000.0, width=W, height=H)
    z = np.load(tmp_path / "lights.npz")
    assert z["lit_mask"].dtype == np.uint64 and z["lit_mask"].tobytes() == lights.lit_mask.tobytes()
    popcount = np.array([bin(int(v)).count("1") for v in lights.lit_mask.ravel()]).reshape(H, W)
    assert np.array_equal(z["lit_count"], popcount) and popcount.max() <= len(LIGHTS) and len(np.unique(popcount)) >= 3
    assert z["dirs"].tobytes() == dirs.tobytes()
    assert z["azimuth_deg"].tolist() == [a for a, _ in LIGHTS] and z["elevation_deg"].tolist() == [e for _, e in LIGHTS]
    assert {k: int(z["stats_" + k]) for k in lights.stats} == lights.stats
    assert f"{len(LIGHTS)} lights: {lights.stats['lit']} point-light pairs lit" in text
