"""The batch router's launches against the recorded trace, without a GPU.

tests/cpp/router_trace.cc links the router's host objects with recording
stand-ins for every kernel launcher and walks a fixed matrix of requests
through tcpck::api::run (and, group P, the FILL front tcpck::api::fill);
tests/golden/router_trace.txt is its
output on the router as it stood before the plan / launch split.  Every
launch, every field of its arguments and every returned status must stay as
recorded: a differing line is a change of behaviour, not something to
regenerate (the recipe and its conditions are in router_trace.cc's header).

The program is built -fsanitize=address,undefined -fno-sanitize-recover=all
(`make -C tcp-stack_amd trace`), so a zero exit status is also a clean
sanitizer run of the router's host code.
"""
import glob
import os
import subprocess

import pytest

from conftest import ROOT

TRACE = os.path.join(ROOT, "tests", "cpp", "build", "router_trace")
GOLDEN = os.path.join(ROOT, "tests", "golden", "router_trace.txt")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def trace_build():
    srcs = [os.path.join(ROOT, "tests", "cpp", "router_trace.cc"), os.path.join(ROOT, "tcp-stack_amd", "Makefile")]
    srcs += glob.glob(os.path.join(ROOT, "tcp-stack_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(TRACE) or max(map(os.path.getmtime, srcs)) > os.path.getmtime(TRACE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tcp-stack_amd"), "-j8", "trace"], check=True)
    return TRACE


def case_key(line):
    """A line's inputs: everything before its launches (a D line: before its count)."""
    return line.split(" ->")[0] if " ->" in line else line.split(" cases=")[0]


def test_router_trace_matches_golden(trace_build):
    r = subprocess.run([trace_build], capture_output=True, text=True, env=ENV, timeout=300, cwd="/tmp")
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert os.path.getsize(GOLDEN) < 512 * 1024
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f"line {i + 1}, case {case_key(w)!r}: the router's launches changed"
                        + (" somewhere in this group (diff `router_trace --all` of both trees)" if w[0] == "D" else "")
                        + f"\n  golden: {w}\n  now:    {g}")
    assert len(got) == len(want), f"{len(got)} lines, golden has {len(want)}"
    # the whole matrix is under the D lines' hashes
    assert sum(int(l.split(" cases=")[1].split()[0]) for l in want if l[0] == "D") > 400000
