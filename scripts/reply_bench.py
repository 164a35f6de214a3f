#!/usr/bin/env python3
"""Batched reply builder (tcpck_batch_reply) against a plain device copy of the
same number of bytes, and against the host loop it replaces.

1M-image rings (the planners' verdict and ack arrays, the demux ids) turned into
the dense ring of 32-B ACK / RST datagrams.  Bytes moved by a call = 1 B of
verdict per image + 4 B of connection id per image when ids are given + per
reply 4 B of ack number read and 36 B written (the 32-B datagram and its source
index).  The templates (32 B per connection, 2 MiB at 64K connections) are
expected to stay in L2 and are not counted, nor is the scratch (4 B per 1024
images).

Workloads: every image replied to; 50 %; 1 %; every image with one connection
(no id array) and with 64K templates under seeded ids; 10 % of the replies RSTs.
Each with device events around every call, 5 warm-up and 20 timed steps, over
`--arrays` sets of input and output arrays taken in turn (8 sets of 1M images
are 360 MB, above the 256 MiB Infinity Cache, so no step reads what the one
before it left there).  In the same process and alternating with it: a torch
copy_ that moves the same number of bytes (half read, half written), over as
many buffers of its own in turn.  On the host: tcpck_build_replies over the
first ring, `--host-steps` timed runs.  Prints each median with its spread, the
rate in moved GB/s, reply / copy in time and host / device.  The first ring's
replies are compared with the host twin's.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tcp-stack_amd")]

import torch  # noqa: E402
import tcpck  # noqa: E402

ROOF_GBS = 8000.0


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def rate(name, ms, nbytes):
    med, lo, hi = float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
    gbs = nbytes / med / 1e6
    print(f"  {name:7s} median {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
          f"{100 * (hi - lo) / med:.1f} %)  {gbs:7.1f} GB/s  {100 * gbs / ROOF_GBS:5.1f} % of the roof", flush=True)
    return med, (hi - lo) / med


def ring(seed, n, p_reply, p_rst, n_conns):
    rng = np.random.default_rng(seed)
    replying = rng.random(n) < p_reply
    rst = rng.random(n) < p_rst
    verdict = np.where(replying, np.where(rst, 16, 7), 1).astype(np.uint8)  # RST / ACCEPT|PAYLOAD|SEND_ACK / ACCEPT
    ack = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    conn = rng.integers(0, n_conns, n, dtype=np.uint64).astype(np.uint32)
    return verdict, ack, conn


def workload(ctx, name, n, p_reply, p_rst, n_conns, with_ids, arrays, warmup, steps, host_steps):
    s = torch.cuda.current_stream()
    tmpl = np.random.default_rng(5).integers(0, 256, 32 * n_conns, dtype=np.uint8)
    d_tmpl = torch.from_numpy(tmpl).cuda()
    scratch = torch.empty(tcpck.reply_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    sets, first = [], None
    for a in range(arrays):
        verdict, ack, conn = ring(100 + a, n, p_reply, p_rst, n_conns)
        if a == 0:
            first = (verdict, ack, conn if with_ids else None)
        sets.append(dict(verdict=torch.from_numpy(verdict).cuda(), ack=torch.from_numpy(ack.view(np.int32)).cuda(),
                         conn=torch.from_numpy(conn.view(np.int32)).cuda() if with_ids else None,
                         replies=torch.empty(32 * n, dtype=torch.uint8, device="cuda"),
                         src=torch.empty(n, dtype=torch.int32, device="cuda"),
                         count=torch.zeros(1, dtype=torch.int64, device="cuda")))
    exp, exp_src, total = tcpck.build_replies(*first[:2], tmpl, conn=first[2], reply_cap=n)
    moved = n * (1 + (4 if with_ids else 0)) + total * (4 + 36)
    half = (moved // 2 + 15) & ~15
    copies = [(torch.randint(0, 255, (half,), dtype=torch.uint8, device="cuda"),
               torch.empty(half, dtype=torch.uint8, device="cuda")) for _ in range(arrays)]

    def call(d):
        ctx.batch_reply(d["verdict"], d["ack"], d_tmpl, n_conns, n, d["replies"], n, d["count"], scratch, conn=d["conn"],
                        src=d["src"], stream=s)

    t_reply, t_copy = [], []
    for i in range(warmup + steps):
        j, jc = i % arrays, (i + arrays // 2) % arrays
        a = timed(lambda: call(sets[j]), s)
        b = timed(lambda: copies[jc][1].copy_(copies[jc][0]), s)
        if i == 0:
            got_total = int(sets[0]["count"].item())
            assert got_total == total, (got_total, total)
            assert np.array_equal(sets[0]["replies"].cpu().numpy()[:32 * total].reshape(-1, 32), exp), "replies differ"
            assert np.array_equal(sets[0]["src"].cpu().numpy()[:total].view(np.uint32), exp_src), "sources differ"
        if i >= warmup:
            t_reply.append(a)
            t_copy.append(b)
    t_host = []
    for _ in range(host_steps):
        t0 = time.perf_counter()
        tcpck.build_replies(*first[:2], tmpl, conn=first[2], reply_cap=n)
        t_host.append((time.perf_counter() - t0) * 1e3)
    print(f"{name}: {n} images, {total} replies, {n_conns} templates, ids {'given' if with_ids else 'NULL'}, "
          f"{arrays} array sets ({arrays * (n * 41 + moved // 2 * 2) / 1e6:.0f} MB), {moved / 1e6:.1f} MB moved per call:",
          flush=True)
    m_r, _ = rate("reply", t_reply, moved)
    m_c, sp_c = rate("copy", t_copy, 2 * half)
    m_h, _ = rate("host", t_host, moved)
    print(f"  reply / copy = {m_r / m_c:.3f} in time (the copy's own spread: {100 * sp_c:.1f} %), "
          f"host / reply = {m_h / m_r:.0f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--arrays", type=int, default=8, help="sets of arrays taken in turn: 8 x 45 MB is above the Infinity Cache")
    args = ap.parse_args()
    ctx = tcpck.Context(0)
    for name, p_reply, p_rst, n_conns, with_ids in (
            ("all reply", 1.0, 0.0, 1024, True), ("50 % reply", 0.5, 0.0, 1024, True), ("1 % reply", 0.01, 0.0, 1024, True),
            ("one connection", 1.0, 0.0, 1, False), ("64K templates", 1.0, 0.0, 65536, True),
            ("10 % RST", 1.0, 0.1, 1024, True)):
        workload(ctx, name, args.images, p_reply, p_rst, n_conns, with_ids, args.arrays, args.warmup, args.steps,
                 args.host_steps)
    ctx.close()


if __name__ == "__main__":
    main()
