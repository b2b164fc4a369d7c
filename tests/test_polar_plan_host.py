"""The planner of the calls along azimuths from the observer (csrc/atmrt_polar_plan.h) on the host, before any entry point trusts it:
tests/csrc/polar_plan_host.cpp, a stand-alone program, runs polar_plan and lattice_steps over the cases this file writes, and every
batch boundary, entries_max and profile offset must be what tests/polar_plan_model.py gives — the two rules restated from the host
code of the commit before the planner.  A second build runs the same cases under the address and undefined-behaviour sanitizers."""
import math
import os
import subprocess

import numpy as np
import pytest

import cbuild
import polar_plan_model as pm

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
HEADER = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc", "atmrt_polar_plan.h")


def _exe(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    return cbuild._build("polar_plan_host.cpp", name, FLAGS + flags)


def _run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    out = [[int(w) for w in row.split()] for row in p.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _plan(row):
    """a plan's line -> (batch_begin, entries_max, off), m"""
    nb = row[0]
    begin, entries_max, n, rest = row[1:1 + nb], row[1 + nb], row[2 + nb], row[3 + nb:]
    assert len(rest) == 2 * n
    return (begin, entries_max, rest[0::2]), rest[1::2]


def uniform_cases():
    for n in (1, 2, 9, 65):
        for m in (1, 33, 300):
            for staged in ([], pm.viewshed_staged(m, False, False, False, False), pm.viewshed_staged(m), pm.HORIZON_STAGED):
                per_az = pm.target_bytes(m) + sum(staged)
                for limit in (1, per_az - 1, per_az, 4 * per_az, 4 * per_az + 255, pm.SCRATCH_BYTES):
                    yield n, m, staged, limit


def greedy_cases():
    ms = [int(v) for v in np.random.default_rng(11).integers(1, 401, size=65)]
    total = sum(pm.target_bytes(m) for m in ms)
    for limit in (1, int(0.4 * total), total, total - 1):
        yield ms, limit


def step_cases():
    """reaches at, one rounding step below and one above d_k (by repeated addition, as the lattice has it) and k * step"""
    for step in (100.0, 0.1, 33.3):
        d, at = 0.0, {}
        for k in range(1, 65537):
            d += step
            at[k] = d
        for k in (1, 2, 7, 300, 4097, 65535, 65536):
            for reach in (at[k], math.nextafter(at[k], 0.0), math.nextafter(at[k], math.inf), k * step):
                yield step, reach


def _check(exe):
    uni, gre, stp = list(uniform_cases()), list(greedy_cases()), list(step_cases())
    assert sum(s == [] for _, _, s, _ in uni) * 4 == len(uni) and {sum(s) for _, m, s, _ in uni if m == 33} == {0, 11 * 33, 39 * 33, 72}
    lines = [f"U {limit} {n} {m} {len(staged)} " + " ".join(map(str, staged)) for n, m, staged, limit in uni]
    lines += [f"G {limit} 0 {len(ms)} " + " ".join(map(str, ms)) for ms, limit in gre]
    lines += [f"S {step.hex()} {reach.hex()} {pm.M_MAX}" for step, reach in stp]
    out = _run(exe, lines)
    several = 0
    for (n, m, staged, limit), row in zip(uni, out):
        got, ms = _plan(row)
        assert ms == [m] * n and got == tuple(pm.uniform(n, m, limit, staged)), (n, m, staged, limit, got)
        several += 1 < pm.batches(got) < n
    assert several > 20  # the sweep holds splits that are neither one batch nor one azimuth to a batch
    counts = []
    for (ms, limit), row in zip(gre, out[len(uni):]):
        got, got_ms = _plan(row)
        assert got_ms == ms and got == tuple(pm.greedy(ms, limit)), (limit, got)
        counts.append(pm.batches(got))
    assert counts == [65, 3, 1, 2]
    refused = 0
    for (step, reach), (got,) in zip(stp, out[len(uni) + len(gre):]):
        want = pm.steps(step, reach)
        assert got == (-1 if want is None else want), (step, reach, got, want)
        refused += want is None
    assert 0 < refused < len(stp)


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_the_planner_gives_the_model_s_batches(opt):
    _check(_exe("polar_plan_host" + opt, [opt]))


def test_65535_samples_are_accepted_and_65536_refused():
    step, d = 100.0, 0.0
    for _ in range(65535):
        d += step
    (a,), (b,) = _run(_exe("polar_plan_host-O2", ["-O2"]), [f"S {step.hex()} {d.hex()} 65535", f"S {step.hex()} {math.nextafter(d, math.inf).hex()} 65535"])
    assert (a, b) == (65535, -1) and pm.steps(step, d) == 65535 and pm.steps(step, math.nextafter(d, math.inf)) is None


def test_the_planner_under_address_and_undefined_behaviour_sanitizers():
    _check(_exe("polar_plan_host_asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_the_header_needs_nothing_of_hip(tmp_path):
    """g++ compiles it alone, with nothing on the include path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return atmrt::lattice_steps(1.0, 2.0, 5) == 2 ? 0 : 1; }\n' % os.path.abspath(HEADER))
    subprocess.run(FLAGS + ["-fsyntax-only", str(src)], check=True)
