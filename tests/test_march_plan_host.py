"""The plan of the first-pass Rectilinear march (csrc/atmrt_march_plan.h) on the host: which of the four routes — plain grid,
small-launch grid, time-sliced march, whole-frame work queue — a launch takes under every ATMRT_MARCH_VARIANT, and the layout of the
time-sliced march's state.  All routes give the same bits, so no frame test can see a launch that takes the wrong one; this test
can.  tests/csrc/march_plan_host.cpp, a stand-alone program, runs march_plan, march_grid_drain and slice_state_layout over the
cases this file writes, and every route, size and offset must be what tests/march_plan_model.py gives.  A second build runs the
same cases under the address and undefined-behaviour sanitizers."""
import itertools
import os
import subprocess

import pytest

import cbuild
import march_plan_model as mm

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
CSRC = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc")
HEADER = os.path.join(CSRC, "atmrt_march_plan.h")

BLOCKS = (0, 1, 60, 6144, 6145, 12288, 12289, 16384, 16385, 32768)
SAMPLES = (0, 126, 127, 600, 2000)
RAGGED = (150 * 61, 2308)  # the "ragged" frame of tests/test_gpu_march_variants.py: pixels, samples


def _exe(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    return cbuild._build("march_plan_host.cpp", name, FLAGS + flags)


def _run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    out = [[int(w) for w in row.split()] for row in p.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def plan_cases():
    """(n, n_t, mode, queue_ok, override)"""
    pixels = [256 * b for b in BLOCKS] + [256 * b - 37 for b in BLOCKS if b]  # the second of each: the same blocks, no multiple of 256
    assert all(mm.blocks(n) in BLOCKS for n in pixels) and sum(n % 256 != 0 for n in pixels) == len(BLOCKS) - 1
    yield from itertools.product(pixels, SAMPLES, (0, 1, 3), (False, True), range(5))
    # the FIFO holds at most 2^31 - 1 entries: a launch of 2048 x 2048 pixels is 65536 groups, which is 32767 slices after the first
    for n_t in (32767 * 128 - 2, 32767 * 128 - 1, 4194302, 4194303):
        yield 2048 * 2048, n_t, 0, False, mm.NONE
        yield 2048 * 2048, n_t, 0, False, mm.SLICED


def grid_cases():
    """(mode, n, override): mode 2 on both sides of its limit, and the queue's fall-back"""
    for mode, b in ((2, 16384), (2, 16385), (0, 16384), (0, 16385)):
        for n in (256 * b, 256 * b - 37):
            for override in range(5):
                yield mode, n, override


def _check(exe):
    plans, grids = list(plan_cases()), list(grid_cases())
    lines = [f"P {n} {n_t} {mode} {int(mode == 3)} {int(q)} {ov}" for n, n_t, mode, q, ov in plans]
    lines += [f"G {mode} {n} {ov}" for mode, n, ov in grids]
    out = _run(exe, lines)
    seen = {mm.NONE: set(), mm.QUEUE: set()}
    for (n, n_t, mode, q, ov), got in zip(plans, out):
        want = mm.route(n, n_t, mode, q, ov)
        assert got[0] == want, (n, n_t, mode, q, ov, got, want)
        sizes = list(mm.slices(n, n_t, mode == 3)) if want == mm.R_SLICED else [0] * 5
        assert got[1:] == sizes, (n, n_t, mode, q, ov, got, sizes)
        if ov in seen:
            seen[ov].add(got[0])
    # a model that agrees with the code on one route only cannot pass
    assert seen[mm.NONE] == seen[mm.QUEUE] == {mm.R_GRID, mm.R_DRAIN, mm.R_SLICED, mm.R_QUEUE}
    for (mode, n, ov), (got,) in zip(grids, out[len(plans):]):
        assert got == mm.grid(mode, n, ov), (mode, n, ov, got)
    by_size = {(mode, mm.blocks(n)): got for (mode, n, ov), (got,) in zip(grids, out[len(plans):]) if ov == mm.NONE}
    assert by_size[2, 16384] == mm.R_DRAIN and by_size[2, 16385] == mm.R_GRID


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_the_plan_gives_the_model_s_routes(opt):
    _check(_exe("march_plan_host" + opt, [opt]))


def test_the_fifo_s_upper_limit():
    """2048 x 2048 pixels: 65536 groups x 32767 slices is the last capacity below 2^31; one sample more is one slice more, and the
    launch (16384 workgroups: small) takes the small-launch grid instead."""
    rows = _run(_exe("march_plan_host-O2", ["-O2"]), [f"P {2048 * 2048} {n_t} 0 0 0 0" for n_t in (32767 * 128 - 2, 32767 * 128 - 1)])
    assert rows[0][0] == mm.R_SLICED and rows[0][4] == 65536 * 32767 <= 0x7FFFFFFF
    assert rows[1] == [mm.R_DRAIN, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("objects", [False, True])
def test_the_slice_state_is_carved_where_the_model_puts_it(objects):
    n, n_t = RAGGED
    (row,) = _run(_exe("march_plan_host-O2", ["-O2"]), [f"L {n} {n_t} {int(objects)}"])
    nbytes, arrays = row[0], [row[1 + 4 * k:5 + 4 * k] for k in range(len(mm.ARRAYS))]
    n_groups, n_pad, after, cap, model_bytes = mm.slices(n, n_t, objects)
    assert nbytes == model_bytes and (n_groups, after) == ((150 * 61 + 63) // 64, (2308 + 2 + 127) // 128)
    if not objects:
        assert nbytes == n_pad * 196 + 64 + 4 * cap
    else:  # what was reserved before the layout and the carving were one code: a whole 256 bytes of padding
        assert nbytes <= n_pad * 196 + 64 + 4 * cap + 256 + n_groups * mm.GROUP_LIST_BYTES
    want = mm.layout(n, n_t, objects)
    spans = []
    for name, (off, size, element, align) in zip(mm.ARRAYS, arrays):
        if name not in want:
            assert name == "glist" and not objects and off == -1
            continue
        assert (off, size) == want[name], (name, off, size, want[name])
        assert (element, align) == mm.ELEMENT[name] and off % align == 0, name  # the block itself begins on 256 bytes
        assert 0 <= off and off + size <= nbytes, name
        spans.append((off, off + size))
    spans.sort()
    assert all(a_end <= b_begin for (_, a_end), (b_begin, _) in zip(spans, spans[1:]))
    assert spans[-1][1] == nbytes  # the layout ends with its last array


def test_the_plan_under_address_and_undefined_behaviour_sanitizers():
    exe = _exe("march_plan_host_asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check(exe)
    n, n_t = RAGGED
    _run(exe, [f"L {n} {n_t} 0", f"L {n} {n_t} 1"])  # every array's first and last byte is written: inside the block of `bytes` bytes


def test_the_header_needs_nothing_but_csrc(tmp_path):
    """g++ compiles it alone, with csrc the only directory on the include path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "atmrt_march_plan.h"\n'
                   "int main() { return atmrt::march_plan(atmrt::MarchShape{256, 600, 0, false, false}, 1).route == atmrt::MarchRoute::Grid ? 0 : 1; }\n")
    subprocess.run(FLAGS + ["-I", os.path.abspath(CSRC), "-fsyntax-only", str(src)], check=True)
