"""atmrt_host::shadow_mask and draw_image_shadowed (include/atmrt_host.hpp) through examples/gen_host.cpp: the status and block the host
program prints for its frame must be the model's (tests/shadow_model.py over the oracle's frame), entry for entry."""
import os
import subprocess

import numpy as np
import pytest

import shadow_model as sm
from atm_raytracer_amd import synth
from test_host_cpp import build_example
from util import run_oracle


def test_host_header_declares_the_shadow_calls(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls them: it must compile and link against the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    example = open(os.path.join(root, "examples", "gen_host.cpp")).read()
    header = open(os.path.join(root, "include", "atmrt_host.hpp")).read()
    assert "shadow_mask(terrain" in example and "draw_image_shadowed(terrain" in example
    assert "inline ShadowMask shadow_mask(" in header and "inline std::vector<uint8_t> draw_image_shadowed(" in header


@pytest.mark.gpu
def test_cpp_shadow_mask_matches_the_model(tmp_path, oracle_det):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    W, H = 40, 24
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", str(W), str(H), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("shadow row")]
    stats = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("shadow stats")]
    image = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("shadow image")]
    assert len(rows) == H and len(stats) == 1 and len(image) == 1
    cfg, _ = synth.scene("S2", W, H, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        want = sm.solve(setting, run_oracle(oracle_det, cfg, tiles), (260.0, 2.0, 20_000.0, 0.0))  # the example's spec
    finally:
        setting.close()
    got = np.array([[tuple(int(v) for v in e.split(":")) for e in f[3].split(",")] for f in rows])
    assert [int(f[2]) for f in rows] == list(range(H)) and got.shape == (H, W, 2)
    got_stats = {k: int(v) for k, v in zip(stats[0][2::2], stats[0][3::2])}
    print(f"shadow host: {got_stats}, model {want.stats_on}; image: {image[0][2:]}")
    assert np.array_equal(got[:, :, 0], want.status) and np.array_equal(got[:, :, 1], want.block)
    assert got_stats == want.stats_on
    assert got_stats["lit"] > 0 and got_stats["shadowed"] > 0
    assert int(image[0][3]) >= 1 and int(image[0][5]) == 0  # shadowed pixels got darker, and only they changed
