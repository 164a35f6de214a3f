"""The receive demultiplexer's host logic under AddressSanitizer + UBSan.

tcp-stack_amd/Makefile `asan` builds tests/cpp/build/demux_host_test
(tests/cpp/demux_host_test.cc, its own main) against libtcpck_asan.so -- the
product library with its HOST code compiled -fsanitize=address,undefined.  The
program runs as a child process with nothing preloaded; a sanitizer report
aborts it (-fno-sanitize-recover=all), so a zero exit status is a clean run.

CPU: a seeded churn of host-only connection tables against a std::map (set,
overwrite, refusal when full, erase with its back-shift, commit's rebuild);
tcpck_plan_deliver_multi on the golden ring and on seeded mixed rings (expected
outputs from tests/demux_np.py plan_multi_np, which tests/test_plan_multi.py
holds against the single planner and the reference's records), every array a
heap block of exactly its size; every TCPCK_EINVAL path.  GPU: one small
create / commit / demux / destroy.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from deliver_np import DeliverGolden
from demux_np import NONE, STATE_KEYS, golden_ring, mixed_ring, plan_multi_np

BUILD = os.path.join(ROOT, "tests", "cpp", "build")
PROGRAM = os.path.join(BUILD, "demux_host_test")
LIB = os.path.join(ROOT, "tcp-stack_amd", "libtcpck_asan.so")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build(built_lib):
    srcs = [os.path.join(ROOT, "tests", "cpp", "demux_host_test.cc")]
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


def ring_lines(hdr, ok, lengths, conn, conns):
    first = [dict(c) for c in conns]
    dst, verdict, ack = plan_multi_np(hdr, ok, conn, lengths, conns)
    out = [f"ring {len(ok)} {len(conns)}"]
    for a, b in zip(first, conns):
        out.append(" ".join(str(int(v)) for v in (
            [a[k] for k in STATE_KEYS] + [a["recv_base"], a["recv_bytes"], a["flags"]] +
            [b["rcv_nxt"], b["snd_una"], b["rcv_wnd"], b["delivered"], b["stopped_at"]])))
    rows = np.asarray(hdr, np.uint8).reshape(-1, 32)
    for k in range(len(ok)):
        out.append(f"{rows[k].tobytes().hex()} {int(ok[k])} {int(lengths[k])} {int(conn[k])} {int(dst[k])} "
                   f"{int(verdict[k])} {int(ack[k])}")
    return out


def test_table_planner_and_argument_checks_cpu(asan_build, tmp_path):
    import tcpck
    lines = []
    dg = DeliverGolden()
    ring = golden_ring(dg, tcpck.update16)
    hdr, ok = dg.host_headers(ring["wire"], ring["offsets"], ring["lengths"])
    s0, s1 = dg.sequences
    conns = [dict({k: s["initial"][k] for k in STATE_KEYS[:4]}, delivered=0, recv_base=b, recv_bytes=s["recv_bytes"],
                  flags=0) for s, b in ((s0, 0), (s1, s0["recv_bytes"] + 64))]
    lines += ring_lines(hdr, ok, ring["lengths"], ring["which"].astype(np.uint32), conns)
    assert [c["delivered"] for c in conns] == [s0["recv_bytes"], s1["recv_bytes"]]
    for seed, n_conns in ((21, 1), (22, 7), (23, 40)):
        hdr, ok, lengths, conn, conns = mixed_ring(seed, n_conns, 80)
        # every fifth connection is the host's, and a tenth of the images find no socket
        for c in conns[4::5]:
            c["flags"] = 1
        conn = conn.copy()
        conn[np.random.default_rng(seed).random(conn.size) < 0.1] = NONE
        lines += ring_lines(hdr, ok, lengths, conn, conns)
    manifest = tmp_path / "demux_manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    out = run([PROGRAM, "cpu", str(manifest)])
    assert out[-1].startswith("ok ") and int(out[-1].split()[1]) > 10000


@pytest.mark.gpu
def test_small_demux_gpu(asan_build):
    out = run([PROGRAM, "gpu"], timeout=300)
    assert out[-1].startswith("ok ")
