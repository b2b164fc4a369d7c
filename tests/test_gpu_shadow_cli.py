"""`gen --shadows` end to end: the image with cast shadows differs from the plain one exactly at SHADOWED pixels and equals there what
the library draws through the Python mirror for the same configuration; --shadow-light naming the Shading light changes nothing."""
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


def test_gen_shadows(gpu_ctx, tmp_path):
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    W, H = 96, 48
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Absolute": 2500.0}},
                    "frame": {"direction": 0.0, "fov": 40.0, "tilt": -6.0, "max_distance": 60000.0},
                    "coloring": {"Shading": {"water_level": 300.0, "ambient_light": 0.3, "light_zenith_angle": 88.0, "light_dir": -80.0}}},
           "simulation_step": 100.0, "output": {"width": W, "height": H, "generator": "Rectilinear"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))

    def gen(out, *extra):
        r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", out, *extra], cwd=str(tmp_path),
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(tmp_path / out).convert("RGB")), r.stdout

    plain, _ = gen("plain.png")
    shadowed, text = gen("shadowed.png", "--shadows", "--shadow-reach", "20000")
    named, _ = gen("named.png", "--shadows", "--shadow-reach", "20000", "--shadow-light", "260", "2")
    # the same through the mirror: light azimuth 0 + 180 - (-80) = 260, elevation 90 - 88 = 2
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain).generate()
    assert generators.light_from_coloring(cfg.params, 88.0, -80.0) == (260.0, 2.0)
    mask = generators.shadow_mask(gpu_ctx, (260.0, 2.0, 20_000.0, 0.0), W, H)
    want = generators.draw_image(gpu_ctx, generators.into_coloring(gpu_ctx.lib, cfg.params, cfg.coloring), W, H, shadows=mask.status)
    sh = mask.status == _abi.SHADOW_SHADOWED
    differ = (shadowed != plain).any(axis=2)
    print(f"shadow cli: {mask.stats}, {int(differ.sum())} pixels differ from the plain image; {text.splitlines()[-3:]}")
    assert f"{mask.stats['lit']} points lit, {mask.stats['shadowed']} in shadow" in text
    assert differ.sum() >= 1 and not differ[~sh].any()
    assert np.array_equal(shadowed[sh], want[sh])
    assert np.array_equal(named, shadowed)
    # the default reach is max_distance: 600 steps here
    _, text = gen("full.png", "--shadows")
    full = generators.shadow_mask(gpu_ctx, (260.0, 2.0, 60_000.0, 0.0), W, H)
    assert f"{full.stats['lit']} points lit, {full.stats['shadowed']} in shadow" in text
