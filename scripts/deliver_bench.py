#!/usr/bin/env python3
"""Receive delivery (tcpck_batch_deliver) against a plain device copy of the
same payload bytes, cold.

Two workloads, every image accepted and in order (destinations back to back):
  * 1M x 1492-B images in 2048-B receive slots;
  * 1M images of the 96 / 608 / 1492 mix in 2048-B slots.
Cold as every key figure here: two arenas and two receive buffers alternated
(each far above the 256 MiB Infinity Cache).  Device events around each call, 5
warm-up and 20 timed steps; in the same process and alternating with it, a
plain device-to-device copy (torch copy_) of the same number of payload bytes,
also between two pairs of buffers.  Algorithmic bytes of a delivery = payload
read + payload written + 8 B of dst per image; of the copy = read + written.
Prints both rates (GB/s and % of the 8 TB/s roof), their ratio and the spread.
--workloads adds jumbo images (jumbo9k: 128K x 9032 B in 9216-B slots; jumbo64k:
16K x 65536 B back to back), measured the same way.
"""
import argparse
import os
import sys

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
    print(f"  {name:8s} median {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
          f"{100 * (hi - lo) / med:.1f} %)  {gbs:7.1f} GB/s  {100 * gbs / ROOF_GBS:5.1f} % of the roof", flush=True)
    return gbs


def workload(ctx, name, lengths, slot, warmup, steps):
    n = lengths.size
    s = torch.cuda.current_stream()
    payload = lengths.astype(np.int64) - 32
    total = int(payload.sum())
    dst = np.concatenate([[0], np.cumsum(payload)[:-1]]).astype(np.uint64)
    d_off = torch.from_numpy(np.arange(n, dtype=np.uint64) * slot).cuda()
    d_len = torch.from_numpy(lengths.astype(np.uint32)).cuda()
    d_dst = torch.from_numpy(dst).cuda()
    arenas = [torch.randint(0, 255, (n * slot,), dtype=torch.uint8, device="cuda") for _ in range(2)]
    recvs = [torch.full((total + 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    srcs = [a[:total] for a in arenas]  # the copy reads as many bytes of the same arenas
    outs = [torch.empty(total, dtype=torch.uint8, device="cuda") for _ in range(2)]
    t_deliver, t_copy = [], []
    for i in range(warmup + steps):
        j = i & 1
        a = timed(lambda: ctx.batch_deliver(arenas[j], n, d_dst, recvs[j], total, offsets=d_off, lengths=d_len,
                                            stream=s), s)
        b = timed(lambda: outs[j].copy_(srcs[j]), s)
        if i >= warmup:
            t_deliver.append(a)
            t_copy.append(b)
    # the delivered stream, checked on a sample of images (and its guard bytes)
    h_recv = recvs[0].cpu().numpy()
    assert (h_recv[total:] == 0xA5).all()
    for k in np.random.default_rng(1).integers(0, n, 2000).tolist() + [0, n - 1]:
        want = arenas[0][k * slot + 32:k * slot + int(lengths[k])].cpu().numpy()
        assert np.array_equal(h_recv[int(dst[k]):int(dst[k]) + want.size], want), k
    print(f"{name}: {n} images, {total / 1e9:.3f} GB of payload", flush=True)
    g_d = rate("deliver", t_deliver, 2 * total + 8 * n)
    g_c = rate("copy", t_copy, 2 * total)
    print(f"  deliver / copy = {g_d / g_c:.3f} in algorithmic bytes per second, "
          f"{float(np.median(t_copy)) / float(np.median(t_deliver)):.3f} in time (copy / deliver)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--workloads", default="fixed,mix", help="of fixed, mix, jumbo9k, jumbo64k")
    args = ap.parse_args()
    ctx = tcpck.Context(0)
    rng = np.random.default_rng(7)
    for w in args.workloads.split(","):
        if w == "fixed":
            workload(ctx, "fixed 1492 B in 2048-B slots", np.full(args.images, 1492), 2048, args.warmup, args.steps)
        elif w == "mix":
            mix = np.asarray((96, 608, 1492))[rng.integers(0, 3, args.images)]
            workload(ctx, "mix 96 / 608 / 1492 B in 2048-B slots", mix, 2048, args.warmup, args.steps)
        elif w == "jumbo9k":
            workload(ctx, "jumbo 9032 B in 9216-B slots", np.full(args.images // 8, 9032), 9216, args.warmup, args.steps)
        elif w == "jumbo64k":
            workload(ctx, "jumbo 65536 B back to back", np.full(args.images // 64, 65536), 65536, args.warmup, args.steps)
        else:
            raise SystemExit(f"unknown workload {w}")
    ctx.close()


if __name__ == "__main__":
    main()
