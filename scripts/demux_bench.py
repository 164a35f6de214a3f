#!/usr/bin/env python3
"""Receive demultiplex (tcpck_batch_demux) against plain device passes over the
same algorithmic bytes.

1M host-order headers (the dense array tcpck_batch_receive writes) looked up in
connection tables of 1, 1K and 64K entries, every image a hit and with 10 % of
the images missing (an address no entry has).  Algorithmic bytes of a demux =
32 B of header read + 4 B of id written per image; the table (16 B per slot, 2
MiB at 64K connections) is expected to stay in L2 and is not counted.

Two residencies, each with device events around every call, 5 warm-up and 20
timed steps:
  * --arrays 2: two header arrays alternated, 75 MB in all -- both stay in the
    256 MiB Infinity Cache, which is how demux meets the array right after
    tcpck_batch_receive wrote it;
  * --arrays 16: sixteen arrays in turn, 604 MB in all, far above the cache:
    every header comes from HBM (cold).
In the same process and alternating with it, two plain passes over the same
arrays:
  * copy:   torch copy_ of 18 B per image (36 B moved per image, as many as a
            demux moves, half read and half written);
  * rowsum: the 8 dwords of every header summed into one dword (32 B read + 4 B
            written per image -- demux's own byte mix, by torch's reduction).
Prints each median, the rate in algorithmic GB/s and the ratio demux / copy in
time.  The ids of the first array are checked against the expected ones.
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
    print(f"  {name:7s} median {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
          f"{100 * (hi - lo) / med:.1f} %)  {gbs:7.1f} GB/s  {100 * gbs / ROOF_GBS:5.1f} % of the roof", flush=True)
    return med


def keys_of(entries):
    """Clustered keys: four host ports, consecutive peer addresses, peer ports that repeat."""
    i = np.arange(entries, dtype=np.uint64)
    return (80 + i % 4).astype(np.uint32), (0x0A000000 + i // 4).astype(np.uint32), (1024 + i % 60000).astype(np.uint32)


def workload(ctx, entries, miss, n, arrays, warmup, steps):
    s = torch.cuda.current_stream()
    host_port, peer_ip, peer_port = keys_of(entries)
    table = tcpck.ConnTable(ctx, entries)
    for i in range(entries):
        table.set(int(host_port[i]), int(peer_ip[i]), int(peer_port[i]), i)
    table.commit()
    d_ip = torch.from_numpy(peer_ip.view(np.int32)).cuda()
    d_ports = torch.from_numpy((peer_port | host_port << 16).view(np.int32)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + entries)
    hdrs, want0 = [], None
    for a in range(arrays):
        h = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 8), dtype=torch.int32, device="cuda", generator=g)
        idx = torch.randint(0, entries, (n,), device="cuda", generator=g)
        missing = torch.rand(n, device="cuda", generator=g) < miss
        h[:, 0] = torch.where(missing, d_ip[idx] ^ (-2 ** 31), d_ip[idx])
        h[:, 3] = d_ports[idx]
        h[:, 6] = (h[:, 6] & ~0x4800) | 0x0800  # ACK, no SYN: the full key
        if a == 0:
            want0 = torch.where(missing, torch.full_like(idx, tcpck.CONN_NONE), idx).cpu().numpy().astype(np.uint32)
        hdrs.append(h)
    conns = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(arrays)]
    halves = [torch.empty(18 * n, dtype=torch.uint8, device="cuda") for _ in range(arrays)]
    t_demux, t_copy, t_sum = [], [], []
    for i in range(warmup + steps):
        # each pass on an array of its own turn, a third of the rotation apart, so that none
        # reads what the pass before it has just brought in (with two arrays all three share one)
        j, jc, js = i % arrays, (i + arrays // 3) % arrays, (i + 2 * (arrays // 3)) % arrays
        a = timed(lambda: ctx.batch_demux(table, hdrs[j], n, conns[j], stream=s), s)
        b = timed(lambda: halves[jc].copy_(hdrs[jc].view(torch.uint8).reshape(-1)[:18 * n]), s)
        c = timed(lambda: torch.sum(hdrs[js], dim=1, dtype=torch.int32, out=conns[js]), s)
        if i == 0:
            ctx.batch_demux(table, hdrs[0], n, conns[0], stream=s)
            torch.cuda.synchronize()
            got = conns[0].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want0), "demux ids differ from the expected ones"
        if i >= warmup:
            t_demux.append(a)
            t_copy.append(b)
            t_sum.append(c)
    slots, _, longest, wrapped = table.stats()
    print(f"{entries} connections ({slots} slots, longest probe {longest}, wrapped {wrapped}), "
          f"{100 * miss:.0f} % misses, {n} images, {arrays} arrays ({arrays * 36 * n / 1e6:.0f} MB):", flush=True)
    m_d = rate("demux", t_demux, 36 * n)
    m_c = rate("copy", t_copy, 36 * n)
    m_s = rate("rowsum", t_sum, 36 * n)
    print(f"  demux / copy = {m_d / m_c:.3f} in time, demux / rowsum = {m_d / m_s:.3f}", flush=True)
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tables", default="1,1024,65536")
    ap.add_argument("--misses", default="0,0.1")
    ap.add_argument("--arrays", default="2,16", help="header arrays taken in turn: 2 stay in the Infinity Cache, 16 do not")
    args = ap.parse_args()
    ctx = tcpck.Context(0)
    for arrays in (int(x) for x in args.arrays.split(",")):
        for entries in (int(x) for x in args.tables.split(",")):
            for miss in (float(x) for x in args.misses.split(",")):
                workload(ctx, entries, miss, args.images, arrays, args.warmup, args.steps)
    ctx.close()


if __name__ == "__main__":
    main()
