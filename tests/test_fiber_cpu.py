"""The host-only core of the scenario batch (activesetmethods_amd/csrc/asm_fiber.h: fiber stacks, fibers, the scheduler's run loop and the
cancellation of a failed round) driven by tests/fiber_host.cpp with a fake round.  The program is a stand-alone C++17 program built with
the undefined-behaviour sanitizer; every case runs as a child process and passes with exit status 0.  This is the only coverage of a failed
round: on a GPU it would take a device failure to get there."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["order", "body_throws", "flush_throws", "guard_page", "two_threads", "cancel_in_destructor"]


@pytest.fixture(scope="module")
def fiber_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ on PATH: tests/fiber_host.cpp cannot be built"
    exe = str(tmp_path_factory.mktemp("fiber") / "fiber_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           "-I", os.path.join(ROOT, "activesetmethods_amd", "csrc"), os.path.join(ROOT, "tests", "fiber_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return exe


@pytest.mark.parametrize("case", CASES)
def test_fiber_scheduler(fiber_host, case):
    r = subprocess.run([fiber_host, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, "case %s: exit status %d\n%s%s" % (case, r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == case + ": ok"
