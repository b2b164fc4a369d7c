"""`gen --sun ... --sky-out` and `gen --refraction-table` end to end: the npz holds the planes of the library's call for the same
configuration, the image shows the sun's colour exactly where `body` is not 0, and the table equals the list call."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

from atm_raytracer_amd import _abi, config, generators, synth
from util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUN_RGB = (255, 244, 214)


def test_gen_sun_and_refraction_table(gpu_ctx, tmp_path):
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

    plain, _ = gen("plain.png")
    sunny, text = gen("sun.png", "--sun", "1.0", "0.8", "--sky-step", "1000", "--sky-out", "sky.npz", "--refraction-table", "table.csv",
                      "--sky-fan", "-1", "9", "11")
    # the same through the mirror
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain).generate()
    sky = generators.sky_directions(gpu_ctx, W, H, step=1000.0)
    body = generators.sky_bodies(gpu_ctx, sky, [generators.sky_body(1.0, 0.8, generators.SUN_RADIUS_DEG, SUN_RGB)])
    data = np.load(tmp_path / "sky.npz")
    print(f"sky cli: {sky.stats}, {int((body != 0).sum())} body pixels; {text.splitlines()[-4:]}")
    assert bits(data["true_elevation"]).tobytes() == bits(sky.true_elevation).tobytes()
    assert data["status"].tobytes() == sky.status.tobytes() and data["steps"].tobytes() == sky.steps.tobytes() and data["body"].tobytes() == body.tobytes()
    assert {k: int(data["stats_" + k]) for k in sky.stats} == sky.stats
    assert 0 < (body != 0).sum() < W * H
    differ = (sunny != plain).any(axis=2)
    assert differ.sum() >= 1 and not differ[body == 0].any()
    assert (sunny[body != 0] == np.array(SUN_RGB, dtype=np.uint8)).all()
    # the table: the list call over the same fan from the observer's altitude
    elev = -1.0 + 10.0 * np.arange(11) / 10
    rec, _ = generators.sky_rays(gpu_ctx, 2500.0, elev, step=1000.0)
    rows = list(csv.reader(open(tmp_path / "table.csv")))
    assert rows[0] == ["elevation_deg", "status", "steps", "true_elevation_deg", "refraction_deg"] and len(rows) == 12
    for row, e, r in zip(rows[1:], elev, rec):
        leaves = int(r["status"]) == _abi.SKY_EXIT
        assert row[:3] == [repr(float(e)), _abi.SKY_STATUS[int(r["status"])], str(int(r["steps"]))]
        assert row[3:] == ([repr(float(r["true_elevation"])), repr(float(e) - float(r["true_elevation"]))] if leaves else ["", ""])
    assert any(row[1] == "exit" for row in rows[1:])
