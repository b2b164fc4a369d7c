"""atmrt_host::viewshed (include/atmrt_host.hpp) through examples/gen_host.cpp: the cells the host program prints must be the model's
(tests/viewshed_model.py), digit for digit."""
import os
import subprocess

import numpy as np
import pytest

import sight_model as sm
import viewshed_model as vm
from atm_raytracer_amd import synth
from test_host_cpp import build_example


def test_host_header_declares_viewshed(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls it: it must compile and link against the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "viewshed(terrain" in open(os.path.join(root, "examples", "gen_host.cpp")).read()


@pytest.mark.gpu
def test_cpp_viewshed_matches_the_model(tmp_path, oracle_det):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", "40", "24", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("viewshed azimuth")]
    print(r.stdout)
    assert len(lines) == 3
    cfg, _ = synth.scene("S2", 40, 24, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        want = vm.solve(setting, 88.0, 2.0, 3, 23_700.0, 0.0, (-6.0, 6.0), 128)
    finally:
        setting.close()
    m = want["d"].size - 1
    for j, f in enumerate(lines):
        v = dict(zip(f[1::2], f[2::2]))
        assert (int(v["azimuth"]), int(v["m"])) == (j, m) == (j, 237)
        for k in ("k_star", "status", "block"):
            assert int(v[k]) == int(want["block_index" if k == "block" else k][j, m - 1]), (j, k)
        for k in ("hidden", "ground", "lat", "lon"):
            a, b = np.float64(v[k]), want[k][j, m - 1]
            assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (j, k, a, b)
