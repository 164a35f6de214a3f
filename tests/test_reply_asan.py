"""The batched reply builder's host code under AddressSanitizer + UBSan.

tcp-stack_amd/Makefile `asan` builds tests/cpp/build/reply_host_test
(tests/cpp/reply_host_test.cc, its own main) against libtcpck_asan.so -- the
product library with its HOST code compiled -fsanitize=address,undefined.  The
program runs as a child process with nothing preloaded; a sanitizer report
aborts it (-fno-sanitize-recover=all), so a zero exit status is a clean run.

CPU: tcpck_build_replies on the fixture ring and on seeded rings (expected
bytes from tests/reply_np.py, which tests/test_reply.py holds against the
reference's datagrams), with and without connection ids, ids that name no
template, reply_cap below and above the total, both modes, every array a heap
block of exactly its size; every TCPCK_EINVAL path.  GPU: one small
tcpck_batch_reply against the host twin.
"""
import glob
import os
import subprocess

import pytest

from conftest import ROOT
from reply_np import ReplyGolden, random_ring, reply_np

BUILD = os.path.join(ROOT, "tests", "cpp", "build")
PROGRAM = os.path.join(BUILD, "reply_host_test")
LIB = os.path.join(ROOT, "tcp-stack_amd", "libtcpck_asan.so")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build(built_lib):
    srcs = [os.path.join(ROOT, "tests", "cpp", "reply_host_test.cc")]
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


def ring_lines(verdict, ack, conn, tmpl, n_conns, cap, mode):
    replies, src, total = reply_np(verdict, ack, conn, tmpl, n_conns, cap, mode)
    out = [f"ring {len(verdict)} {n_conns} {int(conn is not None)} {cap} {mode} {total}"]
    out += [f"{int(verdict[k])} {int(ack[k])} {int(conn[k]) if conn is not None else 0}" for k in range(len(verdict))]
    out += [tmpl[32 * c:32 * c + 32].tobytes().hex() for c in range(n_conns)]
    out += [f"{replies[j].tobytes().hex()} {int(src[j])}" for j in range(len(src))]
    return out


def test_build_replies_and_argument_checks_cpu(asan_build, tmp_path):
    lines = []
    verdict, ack, conn, tmpl = ReplyGolden().ring()
    for mode in (0, 1):
        lines += ring_lines(verdict, ack, conn, tmpl, len(verdict), len(verdict), mode)
    for seed, n, n_conns, bad in ((41, 1, 1, False), (42, 300, 7, False), (43, 900, 40, True), (44, 64, 0, True)):
        verdict, ack, conn, tmpl = random_ring(seed, n, n_conns, bad_ids=bad)
        total = reply_np(verdict, ack, conn, tmpl, n_conns, n, 0)[2]
        for cap in sorted({0, max(total - 1, 0), total, total + 1}):
            lines += ring_lines(verdict, ack, conn, tmpl, n_conns, cap, seed % 2)
        lines += ring_lines(verdict, ack, None, tmpl, n_conns, n, 1 - seed % 2)
    manifest = tmp_path / "reply_manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    out = run([PROGRAM, "cpu", str(manifest)])
    assert out[-1].startswith("ok ") and int(out[-1].split()[1]) > 1000


@pytest.mark.gpu
def test_small_reply_gpu(asan_build):
    out = run([PROGRAM, "gpu"], timeout=300)
    assert out[-1].startswith("ok ")
