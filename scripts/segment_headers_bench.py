#!/usr/bin/env python3
"""Zero-copy segmentation (tcpck_batch_segment_headers) against the two calls it sits between,
on the same bytes.

A 1.5 GB send stream cut at 1460 B (1M segments), in two shapes: one cut, and 256K cuts of four
segments with 7 templates in turn.  Traffic model: the payload is read once and 32 + 14 B are
written per segment (header, offset, length, checksum); the cut table (32 B per cut) and the
templates are overhead.  Baselines, alternating with it in the same process:
  * tcpck_batch_segment, which also writes every image (1504-B slots): time per payload byte;
  * tcpck_batch_fixed(OP_CHECKSUM) over the stream read as packed 1460-B images: the library's own
    read-only rate at this boundary density.
Device events around every call, 5 warm-up and 20 timed steps, cold: two arenas (and two image
buffers) taken in turn, each call on the arena the previous call did not touch, 1.5 GB apiece, far
above the 256 MiB Infinity Cache.  Prints each median with min and max, the share of the 8.0 TB/s
roof under the traffic model, and the ratios.  The first step's checksums of the one-cut shape are
compared with tcpck_batch_segment's.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tcp-stack_amd")]

import torch  # noqa: E402
import tcpck  # noqa: E402

SEG, STRIDE, ROOF = 1460, 1504, 8.0e12


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def show(name, ms, traffic):
    med, lo, hi = float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
    print(f"  {name:14s} median {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  "
          f"{traffic / (med * 1e-3) / ROOF * 100:5.1f} % of the roof over {traffic / 1e6:.0f} MB", flush=True)
    return med


def table(n_seg, per_cut, n_tmpl):
    """Cuts of per_cut segments laid end to end over the stream, templates in turn."""
    n = n_seg // per_cut
    cuts = np.zeros(n, tcpck.send_cut_dtype())
    cuts["offset"] = np.arange(n, dtype=np.uint64) * (per_cut * SEG)
    cuts["bytes"] = per_cut * SEG
    cuts["seq0"] = (12345 + np.arange(n, dtype=np.uint64) * 7919) & 0xFFFFFFFF
    cuts["tmpl"] = np.arange(n) % n_tmpl
    assert tcpck.plan_cuts(cuts, SEG, n_seg * SEG, n_tmpl) == n_seg
    return torch.from_numpy(cuts.view(np.uint8)).cuda(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    n, P = args.segments, args.segments * SEG
    ctx = tcpck.Context(0)
    s = torch.cuda.current_stream()
    tmpl = np.random.default_rng(1).integers(0, 256, (7, 32), dtype=np.uint8)
    d_tmpl = torch.from_numpy(tmpl.reshape(-1)).cuda()
    sets = []
    for a in range(2):
        pay = torch.empty(P, dtype=torch.uint8, device="cuda")
        tcpck.synth_fixed(pay, 1492, 1492, P // 1492, seed=11 + a)  # the stream: a synthetic batch read as flat bytes
        sets.append(dict(pay=pay, images=torch.empty(n * STRIDE, dtype=torch.uint8, device="cuda"),
                         hdr=torch.empty(n * 32, dtype=torch.uint8, device="cuda"),
                         off=torch.empty(n, dtype=torch.int64, device="cuda"),
                         len=torch.empty(n, dtype=torch.int32, device="cuda"),
                         cs=torch.empty(n, dtype=torch.int16, device="cuda"),
                         out=torch.empty(n, dtype=torch.int16, device="cuda")))
    shapes = [("one cut", *table(n, n, 1)), ("256K cuts of 4", *table(n, 4, 7))]

    def headers(d, cuts, n_cuts):
        ctx.batch_segment_headers(d["pay"], P, SEG, cuts, n_cuts, d_tmpl, 7, n, d["hdr"], d["off"], d["len"], d["cs"],
                                  stream=s)

    def segment(d):
        ctx.batch_segment(d["pay"], P, SEG, tmpl[0], 12345, d["images"], STRIDE, d["out"], stream=s)

    def checksum(d):
        ctx.batch_fixed(tcpck.OP_CHECKSUM, d["pay"], SEG, SEG, n, d["out"], stream=s)

    t = {k: [] for k in ("one cut", "256K cuts of 4", "segment", "checksum")}
    for i in range(args.warmup + args.steps):
        row = {}
        for j, (name, cuts, n_cuts) in enumerate(shapes):  # arenas 0, 1, 0, 1: never the one just streamed
            row[name] = timed(lambda: headers(sets[j], cuts, n_cuts), s)
        row["segment"] = timed(lambda: segment(sets[0]), s)
        if i == 0:  # the one-cut shape ran on sets[0] with template 0 and seq0 12345, as segment just did
            assert torch.equal(sets[0]["cs"], sets[0]["out"]), "checksums differ from tcpck_batch_segment's"
        row["checksum"] = timed(lambda: checksum(sets[1]), s)
        if i >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    print(f"{n} segments of {SEG} B, {P / 1e9:.2f} GB of stream, two arenas in turn:", flush=True)
    m = {k: show(k, t[k], P + 46 * n) for k in ("one cut", "256K cuts of 4")}
    m["segment"] = show("segment", t["segment"], P + n * STRIDE + 2 * n)
    m["checksum"] = show("checksum", t["checksum"], P + 2 * n)
    for k in ("one cut", "256K cuts of 4"):
        print(f"  {k}: / segment = {m[k] / m['segment']:.3f}, / checksum = {m[k] / m['checksum']:.3f} in time per payload byte",
              flush=True)
    ctx.close()
    print("one run on one box", flush=True)


if __name__ == "__main__":
    main()
