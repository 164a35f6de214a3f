"""The batched resend pass's host code under AddressSanitizer + UBSan.

tcp-stack_amd/Makefile `asan` builds tests/cpp/build/resend_host_test
(tests/cpp/resend_host_test.cc, its own main) against libtcpck_asan.so -- the
product library with its HOST code compiled -fsanitize=address,undefined.  The
program runs as a child process with nothing preloaded; a sanitizer report
aborts it (-fno-sanitize-recover=all), so a zero exit status is a clean run.

CPU: tcpck_resend_images on the fixture queue and on seeded queues (expected
bytes from tests/resend_np.py, which tests/test_resend.py holds against the
reference's decisions), offset lists and the fixed form, with and without
connection ids, flawed images and ids that name no state, out_cap below and
above the total, both rules and modes, every array a heap block of exactly its
size; every TCPCK_EINVAL path.  GPU: one small tcpck_batch_resend against the
host twin.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from resend_np import ResendGolden, make_queue, resend_np

BUILD = os.path.join(ROOT, "tests", "cpp", "build")
PROGRAM = os.path.join(BUILD, "resend_host_test")
LIB = os.path.join(ROOT, "tcp-stack_amd", "libtcpck_asan.so")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build(built_lib):
    srcs = [os.path.join(ROOT, "tests", "cpp", "resend_host_test.cc")]
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


def queue_lines(q, cap, mode, rule, arena_bytes=None):
    arena = q["arena"][:arena_bytes].copy()
    n, fixed, conn = q["count"], q["offsets"] is None, q["conn"]
    after = arena.copy()
    keep, out_off, out_len, out_conn, src, total = resend_np(
        after, q["snd"], count=n, stride=q["stride"], length=q["length"], offsets=q["offsets"], lengths=q["lengths"],
        conn=conn, cap=cap, rule=rule, mode=mode)
    out = [f"queue {n} {q['snd'].shape[0]} {int(conn is not None)} {int(fixed)} {q['stride']} {q['length']} {arena.size} "
           f"{cap} {mode} {rule} {total}", arena.tobytes().hex()]
    out += [f"{0 if fixed else int(q['offsets'][k])} {0 if fixed else int(q['lengths'][k])} "
            f"{int(conn[k]) if conn is not None else 0}" for k in range(n)]
    out += [f"{int(s[0])} {int(s[1])} {int(s[2])}" for s in q["snd"]]
    out += [after.tobytes().hex(), "".join(str(int(b)) for b in keep) or "-"]
    out += [f"{int(out_off[j])} {int(out_len[j])} {int(out_conn[j])} {int(src[j])}" for j in range(len(src))]
    return out


def test_resend_images_and_argument_checks_cpu(asan_build, tmp_path):
    lines = []
    arena, offsets, lengths, conn, snd = ResendGolden().queue()
    fixture = dict(arena=arena, offsets=offsets, lengths=lengths, conn=conn, snd=snd, stride=0, length=0, count=len(conn))
    for rule in (0, 1):
        lines += queue_lines(fixture, len(conn), 0, rule)
    for seed, n, n_conns, flawed in ((41, 1, 1, False), (42, 300, 7, False), (43, 900, 40, True), (44, 64, 0, True)):
        mode = seed % 2
        q = make_queue(seed, n, n_conns, flaws=flawed, bad_ids=flawed, mode=mode)
        if n_conns == 0:
            q["snd"] = np.zeros((0, 4), np.uint32)
        total = resend_np(q["arena"].copy(), q["snd"], offsets=q["offsets"], lengths=q["lengths"], conn=q["conn"],
                          mode=mode)[5]
        for cap in sorted({0, max(total - 1, 0), total, total + 1}):
            lines += queue_lines(q, cap, mode, 0)
        lines += queue_lines(dict(q, conn=None), n, mode, 1)
        f = make_queue(seed + 10, n, max(n_conns, 1), fixed=True, stride=96, mode=mode)
        lines += queue_lines(f, n, mode, seed % 2)
        lines += queue_lines(f, n, mode, 1 - seed % 2, arena_bytes=max(34, (n - 1) * 96 + 34))  # the last image does not fit
    manifest = tmp_path / "resend_manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    out = run([PROGRAM, "cpu", str(manifest)])
    assert out[-1].startswith("ok ") and int(out[-1].split()[1]) > 200


@pytest.mark.gpu
def test_small_resend_gpu(asan_build):
    out = run([PROGRAM, "gpu"], timeout=300)
    assert out[-1].startswith("ok ")
