#!/usr/bin/env python3
"""Batched resend pass (tcpck_batch_resend) against the parent's call that does the
same work per arena line, tcpck_batch_set_ack with per-image acks, on the same queue.

1M-image send queues of 1492-B images in 2048-B slots (fixed form; one row with
offset lists).  Per image the pass reads the connection id (4 B), the 16-B state
block (the table is expected to stay in L2: 16 B at one connection, 1 MiB at
64K) and one 128-B line of the arena, of which a kept image gets 6 bytes
rewritten; it writes the keep byte to the scratch and to d_keep, and per survivor
20 B of lists (offset 8, length 4, id 4, source 4).  set_ack reads 4 B of ack
number per image and rewrites the same 6 bytes of EVERY image: no predicate, no
lists.  The images' payloads are zero, so the header words alone make a valid
checksum and the survivors could be verified.

Workloads: 100 %, 50 % and 1 % of the queue kept, each with a table of 1 and of
64K connections.  Device events around every call, 5 warm-up and 20 timed steps,
cold: `--arrays` arenas taken in turn (4 arenas touch 4 x 128 MB of lines, above
the 256 MiB Infinity Cache, so no step finds its lines there), the two calls
half a turn apart.  In the same process and alternating with them: a torch copy_
of the list bytes the pass writes (half read, half written).  Prints each median
with min and max, resend / set_ack in time, and resend - (set_ack + copy).  The
first step's count and source list are compared with the mask the queue was built
from.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tcp-stack_amd")]

import torch  # noqa: E402
import tcpck  # noqa: E402

STRIDE, LEN = 2048, 1492


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def show(name, ms):
    med, lo, hi = float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
    print(f"  {name:8s} median {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
    return med


def headers(seed, n, p_keep, snd):
    """n valid 32-B headers (zero payload behind them) and the mask of the owed ones: data images
    whose seq is snd_una + 1 (owed) or snd_una - 5 (acknowledged) of their connection."""
    rng = np.random.default_rng(seed)
    conn = rng.integers(0, snd.shape[0], n, dtype=np.uint64).astype(np.uint32)
    mask = rng.random(n) < p_keep
    hdr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    seq = (snd[conn, 0].astype(np.int64) + np.where(mask, 1, -5)).astype(np.uint32)
    hdr[:, 16:20] = seq.astype(">u4").view(np.uint8).reshape(-1, 4)
    hdr[:, 25] = 0x08
    hdr[:, 10:12] = [(LEN - 32) >> 8, (LEN - 32) & 0xFF]
    hdr[:, 28:30] = 0
    words = hdr.reshape(n, 16, 2).astype(np.uint32)
    s = (words[:, :, 0] | words[:, :, 1] << 8).sum(axis=1)
    hdr[:, 28:30] = (~s & 0xFFFF).astype("<u2").view(np.uint8).reshape(-1, 2)  # REF: the sum mod 2^16
    return hdr, conn, mask


def workload(ctx, arenas, name, n, p_keep, n_conns, lists, warmup, steps):
    s = torch.cuda.current_stream()
    rng = np.random.default_rng(9)
    snd = np.zeros((n_conns, 4), np.uint32)
    snd[:, 0] = rng.integers(16, 1 << 31, n_conns)
    snd[:, 1] = rng.integers(0, 1 << 32, n_conns, dtype=np.uint64)
    d_snd = torch.from_numpy(snd.view(np.int32)).cuda()
    scratch = torch.empty(tcpck.resend_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    d_offsets = torch.arange(n, dtype=torch.int64, device="cuda") * STRIDE if lists else None
    d_lengths = torch.full((n,), LEN, dtype=torch.int32, device="cuda") if lists else None
    sets, first = [], None
    for a, arena in enumerate(arenas):
        hdr, conn, mask = headers(100 + a, n, p_keep, snd)
        if a == 0:
            first = mask
        arena.view(n, STRIDE)[:, :32] = torch.from_numpy(hdr).cuda()
        sets.append(dict(arena=arena, conn=torch.from_numpy(conn.view(np.int32)).cuda(),
                         acks=torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device="cuda"),
                         keep=torch.empty(n, dtype=torch.uint8, device="cuda"),
                         off=torch.empty(n, dtype=torch.int64, device="cuda"),
                         len=torch.empty(n, dtype=torch.int32, device="cuda"),
                         oc=torch.empty(n, dtype=torch.int32, device="cuda"),
                         src=torch.empty(n, dtype=torch.int32, device="cuda"),
                         count=torch.zeros(1, dtype=torch.int64, device="cuda")))
    total = int(first.sum())
    list_bytes = n + 20 * total
    half = (list_bytes // 2 + 15) & ~15
    copies = [(torch.randint(0, 255, (half,), dtype=torch.uint8, device="cuda"),
               torch.empty(half, dtype=torch.uint8, device="cuda")) for _ in arenas]

    def resend(d):
        ctx.batch_resend(d["arena"], n * STRIDE, d_snd, n_conns, n, d["count"], scratch, stride=0 if lists else STRIDE,
                         length=0 if lists else LEN, offsets=d_offsets, lengths=d_lengths, conn=d["conn"], keep=d["keep"],
                         out_offsets=d["off"], out_lengths=d["len"], out_conn=d["oc"], src=d["src"], out_cap=n, stream=s)

    def set_ack(d):
        ctx.batch_set_ack(d["arena"], n, acks=d["acks"], offsets=d_offsets, stride=0 if lists else STRIDE, stream=s)

    t_resend, t_ack, t_copy = [], [], []
    k = len(arenas)
    for i in range(warmup + steps):
        j, ja, jc = i % k, (i + k // 2) % k, (i + 1) % k
        a = timed(lambda: resend(sets[j]), s)
        b = timed(lambda: set_ack(sets[ja]), s)
        c = timed(lambda: copies[jc][1].copy_(copies[jc][0]), s)
        if i == 0:
            assert int(sets[0]["count"].item()) == total, (int(sets[0]["count"].item()), total)
            assert np.array_equal(sets[0]["src"].cpu().numpy()[:total].view(np.uint32), np.flatnonzero(first)), "sources differ"
            assert np.array_equal(sets[0]["keep"].cpu().numpy(), first.astype(np.uint8)), "keep bytes differ"
        if i >= warmup:
            t_resend.append(a)
            t_ack.append(b)
            t_copy.append(c)
    print(f"{name}: {n} images of {LEN} B in {STRIDE}-B slots ({'offset lists' if lists else 'fixed form'}), {total} kept, "
          f"{n_conns} connections, {k} arenas in turn, {list_bytes / 1e6:.1f} MB of keep bytes and lists:", flush=True)
    m_r = show("resend", t_resend)
    m_a = show("set_ack", t_ack)
    m_c = show("copy", t_copy)
    print(f"  resend / set_ack = {m_r / m_a:.2f} in time; resend - (set_ack + copy) = {(m_r - m_a - m_c) * 1e3:.1f} us",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--arrays", type=int, default=4, help="arenas taken in turn: 4 x 128 MB of touched lines is above the Infinity Cache")
    args = ap.parse_args()
    ctx = tcpck.Context(0)
    arenas = [torch.zeros(args.images * STRIDE, dtype=torch.uint8, device="cuda") for _ in range(args.arrays)]
    for name, p_keep, n_conns, lists in (
            ("100 % kept, 1 connection", 1.0, 1, False), ("100 % kept, 64K connections", 1.0, 65536, False),
            ("50 % kept, 1 connection", 0.5, 1, False), ("50 % kept, 64K connections", 0.5, 65536, False),
            ("1 % kept, 1 connection", 0.01, 1, False), ("1 % kept, 64K connections", 0.01, 65536, False),
            ("50 % kept, 64K connections, lists", 0.5, 65536, True)):
        workload(ctx, arenas, name, args.images, p_keep, n_conns, lists, args.warmup, args.steps)
    ctx.close()
    print("one run on one box", flush=True)


if __name__ == "__main__":
    main()
