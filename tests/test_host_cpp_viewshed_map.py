"""atmrt_host::viewshed_map (include/atmrt_host.hpp) through examples/gen_host.cpp: the cells the host program prints must be the model's
(tests/viewshed_map_model.py over the planes of tests/viewshed_model.py), digit for digit."""
import os
import subprocess

import numpy as np
import pytest

import sight_model as sm
import viewshed_map_model as mm
import viewshed_model as vm
from atm_raytracer_amd import synth
from test_host_cpp import build_example


def test_host_header_declares_viewshed_map(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls it: it must compile and link against the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "viewshed_map(terrain" in open(os.path.join(root, "examples", "gen_host.cpp")).read()
    assert "inline ViewshedMap viewshed_map(" in open(os.path.join(root, "include", "atmrt_host.hpp")).read()


@pytest.mark.gpu
def test_cpp_viewshed_map_matches_the_model(tmp_path, oracle_det):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", "40", "24", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cells = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("viewshed_map cell")]
    stats = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("viewshed_map stats")]
    print(r.stdout)
    assert len(cells) == 4 and len(stats) == 1
    cfg, _ = synth.scene("S2", 40, 24, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        v = vm.solve(setting, 88.0, 2.0, 3, 23_700.0, 0.0, (-6.0, 6.0), 128)
    finally:
        setting.close()
    n_samples, n_seen, min_hidden, st = mm.bin_planes((46.25, 8.5, 0.25, 0.25, 2, 2), v["status"], v["hidden"], v["lat"], v["lon"])  # the example's grid
    assert st["n_binned"] == 3 * 237 and (n_samples > 0).sum() >= 2 and st["n_seen"] > 0  # samples north and south of the observer's parallel
    for c, f in enumerate(cells):
        got = dict(zip(f[1::2], f[2::2]))
        assert int(got["cell"]) == c and int(got["n_samples"]) == int(n_samples.ravel()[c]) and int(got["n_seen"]) == int(n_seen.ravel()[c]), (c, got)
        assert np.float64(got["min_hidden"]).tobytes() == min_hidden.ravel()[c].tobytes(), (c, got)
    got = dict(zip(stats[0][2::2], stats[0][3::2]))
    assert {k: int(got[k]) for k in mm.STATS} == st
