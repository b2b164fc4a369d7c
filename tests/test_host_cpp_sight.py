"""atmrt_host::sight_lines (include/atmrt_host.hpp) through examples/gen_host.cpp: the records the host program prints must be the
model's (tests/sight_model.py), digit for digit."""
import subprocess

import numpy as np
import pytest

import sight_model as sm
from atm_raytracer_amd import synth
from test_host_cpp import build_example


def test_host_header_declares_sight_lines(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls it: it must compile and link against the library


@pytest.mark.gpu
def test_cpp_sight_lines_match_the_model(tmp_path, oracle_det):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", "40", "24", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("sight status")]
    print(r.stdout)
    assert len(lines) == 2
    cfg, _ = synth.scene("S2", 40, 24, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        want = sm.solve(setting, [(90.0, 23_700.0, 0.0), (90.0, 23_700.0, 1_800.0)], (-6.0, 6.0), 3)
    finally:
        setting.close()
    got = np.zeros(2, dtype=sm.SIGHT_DTYPE)
    got["block_lat"], got["block_lon"], got["arrival"] = want["block_lat"], want["block_lon"], want["arrival"]  # not printed
    for i, f in enumerate(lines):
        v = dict(zip(f[1::2], f[2::2]))  # "status 1 rounds 3 ..." pairs up to "block"
        got["status"][i], got["rounds_done"][i], got["m"][i] = int(v["status"]), int(v["rounds"]), int(v["m"])
        for k in ("angle", "hidden", "ground", "resolution"):
            got[k][i] = float(v[k])
        got["block_index"][i], got["block_distance"][i], got["block_elevation"][i] = int(f[-3]), float(f[-2]), float(f[-1])
    sm.assert_same(got, want, "gen_host")
    assert set(got["status"].tolist()) <= {sm.SEEN, sm.HIDDEN}
