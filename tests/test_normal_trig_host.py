"""find_normal with the record of its frame constants (csrc/atmrt_core.h: NormalTrig, normal_trig_fill, spherical_calc_from — what
the trace-point epilogue of the kernels reads instead of computing 22 of its 27 sines and cosines again) on the host:
tests/csrc/normal_trig_host.cpp, a stand-alone program, compares it bit for bit with find_normal restated from the primitives that
stay, on 10,000 seeded points and the named edge points over a mosaic with relief placed at six origins, for all four calculators,
both families of world_directions, both divisions and two radii (32 cases per placement), and the factored calculator with
dircalc_new at azimuths 0, 90 and 1,000 seeded ones.  A second build runs the same program under the address and undefined-behaviour
sanitizers.  Host only."""
import re
import subprocess

import cbuild

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math"]


def _run(name, flags):
    p = subprocess.run([cbuild._build("normal_trig_host.cpp", name, FLAGS + flags)], capture_output=True, text=True, timeout=300)
    m = re.search(r"cases (\d+) points (\d+) helper (\d+) failures (\d+)\s*$", p.stdout)
    assert p.returncode == 0 and m, (p.stdout + p.stderr)[-3000:]
    cases, points, helper, failures = map(int, m.groups())
    assert failures == 0, p.stdout[-3000:]
    assert cases == 6 * 32 and points >= 32 * 10_000 and helper == 1002, p.stdout[-300:]


def test_find_normal_with_the_record_equals_the_restated_reference():
    _run("normal_trig_host-O2", ["-O2"])


def test_the_same_under_address_and_undefined_sanitizers():
    _run("normal_trig_host_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
