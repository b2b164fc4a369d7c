"""The rule by which a context keeps what it builds from a frame's inputs (csrc/atmrt_cached.h) on the host, before prepare_frame
trusts it: tests/csrc/cached_host.cpp, a stand-alone program, drives a product with a counting build function.  The first refresh
builds, an equal key does not, a changed key does and the serial grows (A -> B -> A: three builds), `force` builds with an equal key;
a failed build returns its status and leaves the product empty, so that the next refresh builds again whether it asks for the old key
or the new one; a dependent keyed on its source's serial follows a source that failed and was then rebuilt from an equal key, and
only that; keys that differ in 0.0 / -0.0 differ and keys with the same NaN bits are equal.  A second build runs the same program
once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import cbuild

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
HEADER = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc", "atmrt_cached.h")


def _run(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    p = subprocess.run([cbuild._build("cached_host.cpp", name, FLAGS + flags)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip().endswith("failures 0"), (p.stdout + p.stderr)[-3000:]


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_the_cache_rule(opt):
    _run("cached_host" + opt, [opt])


def test_the_cache_rule_under_address_and_undefined_behaviour_sanitizers():
    _run("cached_host_asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_header_needs_nothing_of_hip(tmp_path):
    """g++ compiles it alone, with nothing on the include path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return atmrt::bits(1.0) == atmrt::bits(1.0) ? 0 : 1; }\n' % os.path.abspath(HEADER))
    subprocess.run(FLAGS + ["-fsyntax-only", str(src)], check=True)
