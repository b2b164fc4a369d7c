"""atmrt_host::shadow_lights and the two host functions (include/atmrt_host.hpp) through examples/gen_host.cpp: the mask, the status and
the block planes the host program prints for its frame must be the Python route's over the same frame, byte for byte (and so the
model's: tests/test_gpu_shadow_lights.py)."""
import os
import subprocess

import numpy as np
import pytest

from atm_raytracer_amd import generators, synth
from test_host_cpp import build_example
from util import run_gpu


def test_host_header_declares_the_shadow_light_calls(tmp_path):
    build_example(str(tmp_path / "gen_host"))  # the example calls them: it must compile and link against the library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    example = open(os.path.join(root, "examples", "gen_host.cpp")).read()
    header = open(os.path.join(root, "include", "atmrt_host.hpp")).read()
    assert "shadow_lights(terrain" in example and "shadow_light_direction(" in example and "shadow_local_direction(" in example
    for text in ("inline ShadowLights shadow_lights(", "shadow_light_direction(const atmrt_earth_model_t&", "shadow_local_direction(const atmrt_earth_model_t&"):
        assert text in header, text


@pytest.mark.gpu
def test_cpp_shadow_lights_match_the_python_route(tmp_path, gpu_ctx):
    exe = build_example(str(tmp_path / "gen_host"))
    tiles = synth.synth_tiles([46], [8], level=301)
    synth.write_terrain_dir(str(tmp_path / "terrain"), tiles)
    W, H = 40, 24
    r = subprocess.run([exe, str(tmp_path / "terrain"), "Fast", str(W), str(H), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("lights row")]
    stats = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("lights stats")]
    assert len(rows) == H and len(stats) == 1
    cfg, _ = synth.scene("S2", W, H, generator="Fast", tilt=-2.0, max_distance=60_000.0)  # the example's parameters
    run_gpu(gpu_ctx, cfg, tiles)
    dirs = generators.lights_from_angles(cfg.params, [(260.0, 2.0), (135.0, 30.0)], gpu_ctx.lib)  # the example's lights
    want = generators.shadow_lights(gpu_ctx, dirs, 20_000.0, 0.0, status=True, block=True, width=W, height=H)
    got = np.array([[tuple(int(v) for v in e.split(":")) for e in f[3].split(",")] for f in rows], dtype=np.uint64)
    assert [int(f[2]) for f in rows] == list(range(H)) and got.shape == (H, W, 5)
    got_stats = {k: int(v) for k, v in zip(stats[0][2::2], stats[0][3::2])}
    print(f"shadow lights host: {got_stats}, python {want.stats}")
    assert got[:, :, 0].tobytes() == want.lit_mask.tobytes()
    for l in (0, 1):
        assert got[:, :, 1 + 2 * l].astype(np.uint8).tobytes() == want.status[l].tobytes()
        assert got[:, :, 2 + 2 * l].astype(np.uint16).tobytes() == want.block[l].tobytes()
    assert got_stats == want.stats
    assert got_stats["lit"] > 0 and got_stats["shadowed"] > 0 and len(np.unique(want.lit_mask)) >= 3
