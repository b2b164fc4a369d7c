"""coords_at_dist_sc (csrc/atmrt_core.h), the Spherical geodesic point from a given sin / cos of dist / radius — the form the marching
kernels call with the entries of the per-step table — equals coords_at_dist, and the arithmetic of SphericalCalc::coords_at_dist
written out in the harness, bit for bit on 1e5 seeded (DirCalc, dist) pairs (tests/csrc/coords_sc_host.cpp, a stand-alone host
program); a second build runs a tenth of them under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import cbuild

FLAGS = ["g++", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]


def _run(exe, n):
    p = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    pairs, fast, bad = (int(w) for w in p.stdout.split() if w.isdigit())
    assert pairs == n and bad == 0 and 0.5 * n < fast < n, p.stdout  # both divisions of spherical_sincos were taken


def test_second_form_equals_coords_at_dist():
    _run(cbuild._build("coords_sc_host.cpp", "coords_sc_host", FLAGS + ["-O2"]), 100_000)


def test_second_form_under_address_and_undefined_behaviour_sanitizers():
    exe = cbuild._build("coords_sc_host.cpp", "coords_sc_host_asan_ubsan",
                        FLAGS + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _run(exe, 10_000)
