"""atmrt_host::horizon (include/atmrt_host.hpp) through examples/gen_host.cpp: the records the host program prints must be the model's
(tests/horizon_model.py), digit for digit."""
import os
import subprocess

import numpy as np
import pytest

import horizon_model as hm
import sight_model as sm
from atm_raytracer_amd import synth
from test_host_cpp import build_example


def test_host_header_declares_horizon(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls it: it must compile and link against the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "horizon(terrain" in open(os.path.join(root, "examples", "gen_host.cpp")).read()
    assert "inline std::vector<atmrt_horizon_t> horizon(" in open(os.path.join(root, "include", "atmrt_host.hpp")).read()


@pytest.mark.gpu
def test_cpp_horizon_matches_the_model(tmp_path, oracle_det):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", "40", "24", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("horizon azimuth")]
    print(r.stdout)
    assert len(lines) == 3
    cfg, _ = synth.scene("S2", 40, 24, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        want, _, _ = hm.solve(setting, 88.0, 2.0, 3, 23_700.0, (-6.0, 6.0), 128, 3)
    finally:
        setting.close()
    names = {"status": "status", "rounds": "rounds_done", "k_star": "k_star", "block": "block_index", "clear": "angle_clear", "blocked": "angle_blocked",
             "resolution": "resolution", "distance": "block_distance", "lat": "block_lat", "lon": "block_lon", "elevation": "block_elevation"}
    for j, f in enumerate(lines):
        v = dict(zip(f[1::2], f[2::2]))
        assert int(v["azimuth"]) == j and want["status"][j] == hm.FOUND
        for k, field in names.items():
            if want.dtype[field] == np.int32:
                assert int(v[k]) == int(want[field][j]), (j, k)
            else:
                a, b = np.float64(v[k]), want[field][j]
                assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (j, k, a, b)
