"""The receive delivery entry points' host logic under AddressSanitizer + UBSan.

tcp-stack_amd/Makefile `asan` builds tests/cpp/build/deliver_host_test
(tests/cpp/deliver_host_test.cc, its own main) against libtcpck_asan.so -- the
product library with its HOST code compiled -fsanitize=address,undefined.  The
program runs as a child process with nothing preloaded; a sanitizer report
aborts it (-fno-sanitize-recover=all), so a zero exit status is a clean run.

CPU: tcpck_plan_deliver on the golden arrival sequences and on seeded random
ones (expected outputs from tests/deliver_np.py plan_np, which
tests/test_deliver_plan.py holds against the reference's own results), every
array a heap block of exactly its size, and every TCPCK_EINVAL path of
tcpck_plan_deliver and tcpck_batch_deliver.  GPU: the launcher's arithmetic on
one small delivery.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from deliver_np import DeliverGolden, plan_np, random_arrivals

BUILD = os.path.join(ROOT, "tests", "cpp", "build")
PROGRAM = os.path.join(BUILD, "deliver_host_test")
LIB = os.path.join(ROOT, "tcp-stack_amd", "libtcpck_asan.so")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build(built_lib):
    srcs = [os.path.join(ROOT, "tests", "cpp", "deliver_host_test.cc")]
    srcs += glob.glob(os.path.join(ROOT, "tcp-stack_amd", "csrc", "*"))
    outs = (LIB, PROGRAM)
    if not all(os.path.exists(o) for o in outs) or \
            max(map(os.path.getmtime, srcs)) > min(map(os.path.getmtime, outs)):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tcp-stack_amd"), "-j8", "asan"], check=True)
    return True


def run(args, timeout=300):
    r = subprocess.run(args, capture_output=True, text=True, env=ENV, timeout=timeout, cwd="/tmp")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def sequence_lines(hdr, ok, lengths, state, recv_bytes):
    first = dict(state)
    dst, verdict, ack, consumed = plan_np(hdr, ok, lengths, state, recv_bytes)
    out = ["seq {} {} {} {} {} {} {} {} {} {} {}".format(
        len(ok), recv_bytes, first["rcv_nxt"], first["snd_nxt"], first["snd_una"], first["rcv_wnd"], consumed,
        state["rcv_nxt"], state["snd_una"], state["rcv_wnd"], state["delivered"])]
    rows = np.asarray(hdr, np.uint8).reshape(-1, 32)
    for k in range(len(ok)):
        out.append(f"{rows[k].tobytes().hex()} {int(ok[k])} {int(lengths[k])} {int(dst[k])} {int(verdict[k])} {int(ack[k])}")
    return out


def test_planner_and_argument_checks_cpu(asan_build, tmp_path):
    lines = []
    dg = DeliverGolden()
    for s in dg.sequences:
        hdr, ok = dg.host_headers(dg.wire(s), s["offsets"], s["lengths"])
        state = dict({k: s["initial"][k] for k in ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd")}, delivered=0)
        lines += sequence_lines(hdr, ok, np.asarray(s["lengths"], np.uint32), state, s["recv_bytes"])
        assert state["delivered"] == s["recv_bytes"]
    for seed, rcv_nxt, cap in ((11, 77, 1 << 40), (12, 0xFFFFFFFF - 9000, 1 << 40), (13, 5, 300000)):
        state = dict(rcv_nxt=rcv_nxt, snd_nxt=5000, snd_una=4990, rcv_wnd=7, delivered=0)
        hdr, ok, lengths = random_arrivals(np.random.default_rng(seed), 1500, state)
        lines += sequence_lines(hdr, ok, lengths, state, cap)
    manifest = tmp_path / "deliver_manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    out = run([PROGRAM, "cpu", str(manifest)])
    assert out[-1].startswith("ok ") and int(out[-1].split()[1]) > 1000


@pytest.mark.gpu
def test_small_delivery_gpu(asan_build):
    out = run([PROGRAM, "gpu"], timeout=300)
    assert out[-1].startswith("ok ")
