"""The guided chunks and the priority rule of the whole-frame work queue (csrc/atmrt_march_queue.h: queue_chunk_for with the items
left and the launch's claimers, queue_chunk_cap, queue_items_left, queue_item_priority) on the host, in the
functions the kernel k_rect_march_queue runs: tests/csrc/claim_guided_host.cpp, a stand-alone program, lets 8 and 16 std::threads
of both kinds claim queues of n in {0, 1, 15, 17, 240, 1000} items (and one of 100000) over descending estimates, unguided, with as
many claimers as threads and with the 4096 of a launch; every item must be owned exactly once, a chunk is never 0, never above
MARCH_QUEUE_CHUNK, never above what the steps rule or the cap allows, and 1 once left <= k x claimers.  A second build runs the
same program under ThreadSanitizer.  Host only."""
import os
import subprocess

import cbuild

FLAGS = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"]
HEADER = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc", "atmrt_march_queue.h")


def _run(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    p = subprocess.run([cbuild._build("claim_guided_host.cpp", name, FLAGS + flags)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("failures 0"), (p.stdout + p.stderr)[-3000:]


def test_guided_chunks_own_every_item_once_and_respect_the_cap():
    _run("claim_guided_host-O2", ["-O2"])


def test_guided_chunks_under_thread_sanitizer():
    _run("claim_guided_host_tsan", ["-O1", "-g", "-fsanitize=thread"])
