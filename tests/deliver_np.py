"""numpy restatements of the receive delivery path, for the tests.

plan_np:    tcpck_plan_deliver -- SocketInternal::RecvPacket
            (socket-internal.h:161-171) then Estab::operator()(const TcpHeader &,
            ...) (state.cc:195-223) over an arrival sequence of host-order headers.
deliver_np: tcpck_batch_deliver -- Accept()'s append (socket-internal.h:323-334)
            as a scatter of payload ranges into a receive buffer.
"""
import json
import os

import numpy as np

SKIP = 0xFFFFFFFFFFFFFFFF
MAX_LEN = 1 << 24  # a longer image is no TCP image: tcpck_batch_deliver skips it
ACCEPT, PAYLOAD, SEND_ACK, BAD_SUM = 1, 2, 4, 8
F_ACK, F_SYN, F_FIN = 0x08, 0x40, 0x80  # header byte 25, the reference's bits (tcp-header.h:122-162)
M32 = 0xFFFFFFFF


def header_fields(hdr):
    """(tcp_length, seq, ack, flags, window) arrays of 32-B host-order headers."""
    h = np.ascontiguousarray(hdr, np.uint8).reshape(-1, 32)
    u16 = lambda at: h[:, at].astype(np.int64) | (h[:, at + 1].astype(np.int64) << 8)
    u32 = lambda at: u16(at) | (u16(at + 2) << 16)
    return u16(10), u32(16), u32(20), h[:, 25].astype(np.int64), u16(26)


def plan_np(hdr, ok, lengths, state, recv_bytes):
    """state: dict rcv_nxt, snd_nxt, snd_una, rcv_wnd, delivered (updated in place).
    Returns (dst u64[n], verdict u8[n], ack u32[n], consumed)."""
    tl, seq, ack, flags, win = header_fields(hdr)
    n = len(ok)
    dst = np.full(n, SKIP, np.uint64)
    verdict = np.zeros(n, np.uint8)
    reply = np.zeros(n, np.uint32)
    k = 0
    while k < n:
        if not ok[k]:
            verdict[k] = BAD_SUM | SEND_ACK
            reply[k] = state["rcv_nxt"]
            k += 1
            continue
        in_order = ack[k] <= state["snd_nxt"] and seq[k] == state["rcv_nxt"]
        kind = int(flags[k]) & (F_ACK | F_SYN | F_FIN)
        if in_order and kind == (F_ACK | F_FIN):
            break
        if in_order and kind == F_ACK:
            payload = int(lengths[k]) - 32
            append = tl[k] > 0 and payload > 0
            if append and state["delivered"] + payload > recv_bytes:
                break
            state["snd_una"] = max(int(ack[k]), state["snd_una"])
            state["rcv_nxt"] = (int(seq[k]) + int(tl[k])) & M32
            state["rcv_wnd"] = int(win[k])
            verdict[k] = ACCEPT | (SEND_ACK if tl[k] > 0 else 0) | (PAYLOAD if append else 0)
            if append:
                dst[k] = state["delivered"]
                state["delivered"] += payload
        reply[k] = state["rcv_nxt"]
        k += 1
    reply[k:] = state["rcv_nxt"]
    return dst, verdict, reply, k


def deliver_np(arena, offsets, lengths, dst, recv):
    """recv (a uint8 array, changed in place and returned) after tcpck_batch_deliver
    (include/tcpck.h): an image whose dst is SKIP or odd, whose range does not fit, whose
    length or offset is odd, or whose length is below 32 or above 16 MiB is skipped whole
    (a length of 32 has no payload)."""
    for off, ln, d in zip(np.asarray(offsets, np.uint64).tolist(), np.asarray(lengths, np.int64).tolist(),
                          np.asarray(dst, np.uint64).tolist()):
        p = ln - 32
        if d == SKIP or d & 1 or ln & 1 or off & 1 or ln < 32 or ln > MAX_LEN or p <= 0 or d + p > recv.size:
            continue
        recv[d:d + p] = arena[off + 32:off + ln]
    return recv


def deliver_np_fast(arena, offsets, lengths, dst, recv, chunk=1 << 22):
    """deliver_np without the per-image loop, for counts in the hundreds of thousands: the
    delivered images' payload bytes as one gather / scatter over np.repeat'ed per-byte
    indices, `chunk` bytes at a time.  Like the device (and unlike the loop, which lets the
    later image win) it leaves overlapping destination ranges unspecified."""
    off = np.asarray(offsets, np.uint64)
    ln = np.asarray(lengths, np.int64)
    d = np.asarray(dst, np.uint64)
    p = ln - 32
    size = np.uint64(recv.size)
    ok = (d != np.uint64(SKIP)) & ((d & np.uint64(1)) == 0) & ((off & np.uint64(1)) == 0) & ((ln & 1) == 0)
    ok &= (ln > 32) & (ln <= MAX_LEN) & (d <= size)  # (d <= size first: d + p cannot wrap below)
    ok[ok] = d[ok] + p[ok].astype(np.uint64) <= size
    src, at, p = off[ok].astype(np.int64) + 32, d[ok].astype(np.int64), p[ok]
    ends = np.cumsum(p)
    lo = 0
    while lo < p.size:  # whole images per round, at least one
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + chunk, side="right")))
        n = p[lo:hi]
        first = np.repeat(ends[lo:hi] - n, n)   # per byte: where its image's bytes start in this round's run
        within = np.arange((ends[lo - 1] if lo else 0), ends[hi - 1]) - first
        recv[np.repeat(at[lo:hi], n) + within] = arena[np.repeat(src[lo:hi], n) + within]
        lo = hi
    return recv


def random_arrivals(rng, n, state):
    """Header-space arrival sequence: a sender's segments with duplicates, gaps, damage and flag noise."""
    hdr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lengths = np.empty(n, np.uint32)
    ok = np.ones(n, np.uint8)
    seq, segs, need = state["rcv_nxt"], [], 0  # need: the first segment not accepted yet

    def seg(i):
        nonlocal seq
        while len(segs) <= i:
            p = int(rng.choice([0, 0, 2, 16, 100, 536, 1460, 9000]))
            tl = p if rng.random() < 0.9 else int(rng.integers(0, 70))
            segs.append((seq, p, tl))
            seq = (seq + tl) & 0xFFFFFFFF
        return segs[i]

    k = 0
    while k < n:
        r = rng.random()
        i = need if r < 0.6 else (need + int(rng.integers(1, 4)) if r < 0.8 else max(0, need - int(rng.integers(1, 4))))
        pick = seg(i)
        s, p, tl = pick
        r = rng.random()
        flags = 0x08 | (int(rng.integers(0, 256)) & 0x34)  # ACK + noise in URG / PSH / RST
        if r < 0.04:
            flags &= ~0x08
        elif r < 0.08:
            flags |= 0x40
        elif r < 0.09:
            flags |= 0x80  # a FIN: in sequence it stops the walk
        ack = state["snd_nxt"] - int(rng.integers(0, 3)) if rng.random() < 0.93 else state["snd_nxt"] + int(rng.integers(1, 9))
        if rng.random() < 0.05:
            s = (s + int(rng.integers(1, 3000))) & 0xFFFFFFFF  # a hole
        h = hdr[k]
        h[10:12] = np.frombuffer(int(tl).to_bytes(2, "little"), np.uint8)
        h[16:20] = np.frombuffer(int(s).to_bytes(4, "little"), np.uint8)
        h[20:24] = np.frombuffer(int(ack & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        h[25] = flags
        lengths[k] = 32 + p
        ok[k] = rng.random() > 0.06
        if i == need and s == pick[0] and ok[k] and flags & 0xC8 == 0x08 and ack <= state["snd_nxt"]:
            need += 1
        k += 1
    return hdr.reshape(-1), ok, lengths


class DeliverGolden:
    """tests/golden/deliver_golden.{bin,json}: arrival sequences fed to the
    reference's TcpStateManager in Estab with a recording SocketInternalInterface
    (tests/golden/gen_deliver.cc): per image the verdict bits, whether Accept()
    appended, the reply ACK; the control block before and after; the final
    recv_buffer."""

    def __init__(self):
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "deliver_golden.json")) as f:
            meta = json.load(f)
        self.blob = np.fromfile(os.path.join(here, meta["blob"]), dtype=np.uint8)
        assert self.blob.size == meta["blob_bytes"]
        self.sequences = meta["sequences"]

    def wire(self, s):
        return self.blob[s["wire_off"]:s["wire_off"] + s["arena_bytes"]].copy()

    def recv(self, s):
        return self.blob[s["recv_off"]:s["recv_off"] + s["recv_bytes"]].copy()

    @staticmethod
    def host_headers(wire, offsets, lengths):
        """The dense host-order header array and verdicts tcpck_batch_receive writes (numpy)."""
        from oracle.ref16 import receive_np
        host = wire.copy()
        ok = receive_np(host, np.asarray(offsets, np.int64), np.asarray(lengths, np.uint32))
        hdr = np.concatenate([host[o:o + 32] for o in np.asarray(offsets).tolist()]) if len(offsets) else np.zeros(0, np.uint8)
        return hdr, ok
