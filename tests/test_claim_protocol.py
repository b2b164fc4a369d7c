"""The claim arithmetic of the whole-frame work queue (csrc/atmrt_march_queue.h: one 64-bit word `head | tail << 32`, long claimers
add 1 and own the head item, short claimers add C << 32 and own a chunk below the tail) on the host, in the functions the kernel
k_rect_march_queue runs: tests/csrc/claim_host.cpp, a stand-alone program, lets 8 and 16 std::threads of mixed roles claim queues of
n in {0, 1, 15, 16, 17, 1000} items with C in {1, 16} (and one of 100000) and walks every short interleaving by hand; every item
must be owned exactly once, no claim may leave 0 .. n-1, and a claim after the queue ran empty owns nothing.  A second build runs
the same program under ThreadSanitizer."""
import os
import subprocess

import cbuild

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"]
HEADER = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc", "atmrt_march_queue.h")


def _run(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    p = subprocess.run([cbuild._build("claim_host.cpp", name, FLAGS + flags)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("failures 0"), (p.stdout + p.stderr)[-3000:]


def test_every_item_is_claimed_once():
    _run("claim_host-O2", ["-O2"])


def test_every_item_is_claimed_once_under_thread_sanitizer():
    _run("claim_host_tsan", ["-O1", "-g", "-fsanitize=thread"])


def test_the_header_needs_nothing_of_hip(tmp_path):
    """g++ compiles it alone, with nothing on the include path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { unsigned f; return (int)atmrt::queue_claim_items(0, true, 16, 0, f); }\n' % os.path.abspath(HEADER))
    subprocess.run(FLAGS + ["-fsyntax-only", str(src)], check=True)
