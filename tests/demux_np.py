"""numpy / Python restatements of the receive demultiplexer, for the tests.

demux_np:      tcpck_batch_demux -- SocketManager::ReceivePacket's lookup
               (socket-manager.h:187-196) on host-order headers against a dict.
plan_multi_np: tcpck_plan_deliver_multi -- built on deliver_np.plan_np, one
               image at a time, with the no-socket branch (socket-manager.h:
               197-207) and the hand-over to the host state machine.
mixed_ring:    seeded arrival sequences of many connections interleaved in one ring.
golden_ring:   the two sequences of tests/golden/deliver_golden.* as two
               connections interleaved in one ring.
"""
import numpy as np

from deliver_np import F_ACK, F_SYN, SKIP, plan_np, random_arrivals

NONE = 0xFFFFFFFF
NOT_STOPPED = 0xFFFFFFFFFFFFFFFF
CONN_HOST = 1
RST, HOST = 16, 32
STATE_KEYS = ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd", "delivered")


def header_keys(hdr):
    """(host_port, peer_ip, peer_port, flags) arrays of 32-B host-order headers: the source
    address is the u32 at byte 0, the source / destination port the u16 at 12 / 14."""
    h = np.ascontiguousarray(hdr, np.uint8).reshape(-1, 32).astype(np.int64)
    ip = h[:, 0] | h[:, 1] << 8 | h[:, 2] << 16 | h[:, 3] << 24
    return h[:, 14] | h[:, 15] << 8, ip, h[:, 12] | h[:, 13] << 8, h[:, 25]


def demux_np(hdr, table):
    """table: {(host_port, peer_ip, peer_port): id}.  The three key rules: the host address is
    not part of the key (the destination address is never read); SYN without ACK looks up the
    listener (host_port, 0, 0); everything else the full key, compared exactly."""
    host_port, peer_ip, peer_port, flags = header_keys(hdr)
    out = np.full(host_port.size, NONE, np.uint32)
    for k in range(host_port.size):
        if flags[k] & (F_SYN | F_ACK) == F_SYN:
            key = (int(host_port[k]), 0, 0)
        else:
            key = (int(host_port[k]), int(peer_ip[k]), int(peer_port[k]))
        out[k] = table.get(key, NONE)
    return out


def plan_multi_np(hdr, ok, conn, lengths, conns):
    """conns: list of dicts with STATE_KEYS, recv_base, recv_bytes, flags (updated in place;
    stopped_at is set).  Returns (dst u64[n], verdict u8[n], ack u32[n])."""
    rows = np.ascontiguousarray(hdr, np.uint8).reshape(-1, 32)
    n = len(ok)
    dst = np.full(n, SKIP, np.uint64)
    verdict = np.zeros(n, np.uint8)
    ack = np.zeros(n, np.uint32)
    for c in conns:
        c["stopped_at"] = NOT_STOPPED
    host_seen = False
    for k in range(n):
        if conn[k] == NONE:
            if ok[k]:
                verdict[k] = HOST if host_seen else RST
                if not host_seen:
                    ack[k] = int.from_bytes(rows[k, 20:24].tobytes(), "little")
            continue
        c = conns[int(conn[k])]
        if c["flags"] & CONN_HOST:
            verdict[k], ack[k], host_seen = HOST, c["rcv_nxt"], True
            continue
        if c["stopped_at"] == NOT_STOPPED:
            d, v, a, used = plan_np(rows[k], ok[k:k + 1], lengths[k:k + 1], c, c["recv_bytes"])
            if used:
                verdict[k], ack[k] = v[0], a[0]
                if d[0] != SKIP:
                    dst[k] = c["recv_base"] + int(d[0])
                continue
            c["stopped_at"] = k
        ack[k] = c["rcv_nxt"]
    return dst, verdict, ack


def interleave(rng, counts):
    """A ring order over len(counts) sequences: which[k] = the sequence of ring slot k, idx[k] =
    that image's index within its sequence (each sequence's own order is kept)."""
    which = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    idx = np.zeros(which.size, np.int64)
    for c in range(len(counts)):
        at = np.flatnonzero(which == c)
        idx[at] = np.arange(at.size)
    return which, idx


def mixed_ring(seed, n_conns, per_conn):
    """n_conns seeded arrival sequences interleaved in one ring; small windows for some, rcv_nxt
    near 2^32 for some."""
    rng = np.random.default_rng(seed)
    conns, parts, base = [], [], 0
    for c in range(n_conns):
        rcv_nxt = int(rng.choice([1000, 0xFFFFFFFF - 20000, 0xFFFFFFFF - 100, 0x7FFFFFF0]))
        recv_bytes = int(rng.choice([3000, 20000, 1 << 30]))
        st = dict(rcv_nxt=rcv_nxt, snd_nxt=5000, snd_una=4990, rcv_wnd=7, delivered=0, recv_base=base,
                  recv_bytes=recv_bytes, flags=0)
        base += min(recv_bytes, 1 << 20) + 2 * int(rng.integers(0, 40))
        parts.append(random_arrivals(rng, int(rng.integers(per_conn // 2, per_conn + 1)), st))
        conns.append(st)
    which, idx = interleave(rng, [p[1].size for p in parts])
    hdr = np.stack([parts[c][0].reshape(-1, 32)[i] for c, i in zip(which, idx)]).reshape(-1)
    ok = np.asarray([parts[c][1][i] for c, i in zip(which, idx)], np.uint8)
    lengths = np.asarray([parts[c][2][i] for c, i in zip(which, idx)], np.uint32)
    return hdr, ok, lengths, which.astype(np.uint32), conns


def set_port(wire, off, at, port, update16):
    """The big-endian u16 at wire bytes [off + at, + 2) := port, the stored checksum (bytes
    28-29, a little-endian word as the reference sums them) updated, so the verdict stays."""
    old = int(wire[off + at]) | int(wire[off + at + 1]) << 8
    wire[off + at], wire[off + at + 1] = port >> 8, port & 0xFF
    new = int(wire[off + at]) | int(wire[off + at + 1]) << 8
    cs = update16(int(wire[off + 28]) | int(wire[off + 29]) << 8, old, new)
    wire[off + 28], wire[off + 29] = cs & 0xFF, cs >> 8


PORT_1 = 15502  # sequence 1's source port in the ring


def golden_ring(dg, update16, seed=5):
    """The fixture's two arrival sequences as connections 0 and 1 of one ring: one arena (sequence
    1's bytes after sequence 0's), sequence 1's source port rewritten to PORT_1 with the checksum
    adjusted, the images interleaved by a seeded shuffle that keeps each sequence's order.
    Returns a dict: wire, offsets, lengths, which, idx."""
    s0, s1 = dg.sequences
    w1 = dg.wire(s1)
    for off in s1["offsets"]:
        set_port(w1, off, 12, PORT_1, update16)
    wire = np.concatenate([dg.wire(s0), w1])
    base = [0, s0["arena_bytes"]]
    assert base[1] % 2 == 0
    which, idx = interleave(np.random.default_rng(seed), [len(s0["offsets"]), len(s1["offsets"])])
    seqs = (s0, s1)
    offsets = np.asarray([base[c] + seqs[c]["offsets"][i] for c, i in zip(which, idx)], np.uint64)
    lengths = np.asarray([seqs[c]["lengths"][i] for c, i in zip(which, idx)], np.uint32)
    return dict(wire=wire, offsets=offsets, lengths=lengths, which=which, idx=idx)


def check_golden_ring(dg, ring, hdr, ok, conn, dst, verdict, ack, conns):
    """The multi planner's outputs on the golden ring against the reference's per-image records
    (tests/golden/gen_deliver.cc), as tests/test_deliver_plan.py reads them for one sequence.
    conns: two objects or dicts with the final control blocks; returns nothing."""
    from deliver_np import ACCEPT, BAD_SUM, PAYLOAD, SEND_ACK
    get = (lambda c, k: c[k]) if isinstance(conns[0], dict) else (
        lambda c, k: getattr(c, k) if hasattr(c, k) else getattr(c.rcv, k))
    for c, s in enumerate(dg.sequences):
        at_ring = np.flatnonzero(ring["which"] == c)
        n = len(s["offsets"])
        assert at_ring.size == n and (conn[at_ring] == c).all()
        assert ok[at_ring].tolist() == s["ok"]
        stop = s["left_estab_at"] if s["left_estab_at"] >= 0 else n
        assert get(conns[c], "stopped_at") == (at_ring[stop] if stop < n else NOT_STOPPED)
        at = 0
        for i, k in enumerate(at_ring):
            if i >= stop:
                assert verdict[k] == 0 and dst[k] == SKIP
                continue
            if not s["ok"][i]:
                want = BAD_SUM | SEND_ACK
            elif s["accepted"][i]:
                want = ACCEPT | (SEND_ACK if s["send_ack"][i] else 0) | (PAYLOAD if s["appended"][i] else 0)
            else:
                want = 0
            assert verdict[k] == want, (c, i, verdict[k], want)
            if s["send_ack"][i]:
                assert ack[k] == s["reply_ack"][i], (c, i)
            if s["appended"][i]:
                assert dst[k] == get(conns[c], "recv_base") + at
                at += s["appended"][i]
            else:
                assert dst[k] == SKIP
        assert at == s["recv_bytes"] == get(conns[c], "delivered")
        for key in ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd"):
            assert get(conns[c], key) == s["final"][key], (c, key)
