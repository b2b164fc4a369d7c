"""`gen --sight-lines FILE.csv` end to end: a three-row CSV in, three rows with the documented columns out, equal to what the library
returns for the same targets through the Python mirror."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from atm_raytracer_amd import _abi, config, generators, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_sight_lines(gpu_ctx, tmp_path):
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 90.0, "fov": 30.0, "tilt": 0.0, "max_distance": 60000.0}},
           "simulation_step": 100.0, "output": {"width": 96, "height": 48, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    # a valley floor 23.7 km east of the observer, a 1800 m mast on it, and a place 5 km to the north (outside the frame)
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain)._configure()
    east = [float(v[0]) for v in generators.coords_at_dist(gpu_ctx, 46.5, 8.5, 90.0, [23_700.0])]  # plain floats: their repr goes into the CSV
    north = [float(v[0]) for v in generators.coords_at_dist(gpu_ctx, 46.5, 8.5, 0.0, [5_000.0])]
    names = ["floor", "mast, quoted", "north"]
    lat, lon, height = [east[0], east[0], north[0]], [east[1], east[1], north[1]], [None, 1800.0, 10.0]
    with open(tmp_path / "targets.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "lat", "lon", "height"])
        for n, a, b, h in zip(names, lat, lon, height):
            w.writerow([n, repr(a), repr(b)] + ([] if h is None else [repr(h)]))
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--sight-lines", "targets.csv",
                        "--sight-out", "sights.csv", "--sight-fan", "-6", "6", "--sight-rounds", "2"], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(tmp_path / "sights.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == generators.SIGHT_COLUMNS and len(rows) == 4
    targets = generators.sight_targets(gpu_ctx, np.array(lat), np.array(lon), np.array([0.0, 1800.0, 10.0]))
    want = generators.sight_lines(gpu_ctx, targets, (-6.0, 6.0), 2)
    print("sight cli:", rows[1:], want)
    for row, name, t, s in zip(rows[1:], names, targets, want):
        d = dict(zip(generators.SIGHT_COLUMNS, row))
        assert d["name"] == name and float(d["azimuth_deg"]) == t["azimuth_deg"] and float(d["distance_m"]) == t["distance"]
        assert d["status"] == _abi.SIGHT_STATUS[int(s["status"])]
        for col, field in (("angle_deg", "angle"), ("hidden_m", "hidden"), ("ground_m", "ground"), ("resolution_deg", "resolution"),
                           ("block_distance_m", "block_distance"), ("block_lat", "block_lat"), ("block_lon", "block_lon"),
                           ("block_elevation_m", "block_elevation")):
            assert d[col] == ("" if np.isnan(s[field]) else repr(float(s[field]))), (name, col)
        px = generators.fast_pixel_of(cfg.params, float(t["azimuth_deg"]), float(s["angle"]))
        assert (d["x"], d["y"]) == (("", "") if px is None else (str(px[0]), str(px[1])))
    assert abs(targets["azimuth_deg"][0] - 90.0) < 1e-6 and abs(targets["distance"][0] - 23_700.0) < 1e-3
    by_name = {row[0]: dict(zip(generators.SIGHT_COLUMNS, row)) for row in rows[1:]}
    assert by_name["floor"]["status"] == "hidden" and by_name["floor"]["block_distance_m"] != "" and by_name["mast, quoted"]["status"] in ("seen", "hidden")
    assert by_name["mast, quoted"]["x"] == "48" and by_name["north"]["x"] == ""  # due east is the middle column; north is outside the 30 degree frame
