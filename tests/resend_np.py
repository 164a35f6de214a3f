"""numpy restatement of the batched resend pass, for the tests.

resend_np:     tcpck_batch_resend / tcpck_resend_images (include/tcpck.h) -- the reference's
               resend event (ResendPredicate, socket-internal.h:363-390) over a whole send queue,
               vectorised: the predicate per image here, the patch of the kept subset by
               oracle.ref16.resend_batch_np (the ACK rewrite and SendPacket's FULL recompute).
ResendGolden:  tests/golden/resend_golden.{bin,json}: images, states, keep decisions and patched
               headers made by the reference's own helpers (tests/golden/gen_resend.cc).
make_queue:    a seeded send queue of valid images for the twin / device comparisons.
"""
import json
import os

import numpy as np

from oracle.ref16 import ref16_batch_np, resend_batch_np, segment_np

NONE = 0xFFFFFFFF
CLOSED = 1
RULE_REF, RULE_SERIAL = 0, 1
SYN, FIN, ACK = 0x40, 0x80, 0x08


def fill_batch_np(arena, offsets, lengths, mode=0):
    """SendPacket's two checksum lines on every image, in place (disjoint images)."""
    offsets = np.asarray(offsets, np.int64)
    if offsets.size == 0:
        return
    fld = offsets[:, None] + np.arange(28, 30)[None, :]
    arena[fld] = 0
    c = ref16_batch_np(arena, offsets, np.asarray(lengths, np.int64), mode)
    arena[fld] = c.astype("<u2").view(np.uint8).reshape(-1, 2)


def _be(arena, at, width):
    """Big-endian unsigned of `width` bytes at each index of `at`."""
    v = np.zeros(at.size, np.uint64)
    for i in range(width):
        v = (v << np.uint64(8)) | arena[at + i].astype(np.uint64)
    return v


def keep_np(arena, snd, offsets, lengths, conn, rule):
    """The keep decision per image (bool).  offsets / lengths: one entry per image; conn: ids or
    None; snd: uint32[n_conns, 4] rows of (snd_una, rcv_nxt, flags, reserved)."""
    offsets = np.asarray(offsets, np.uint64)
    lengths = np.asarray(lengths, np.uint64)
    n = offsets.size
    snd = np.asarray(snd, np.uint32).reshape(-1, 4)
    c = np.zeros(n, np.uint64) if conn is None else np.asarray(conn, np.uint32).astype(np.uint64)
    size = np.uint64(arena.size)
    ok = (offsets % 2 == 0) & (lengths % 2 == 0) & (lengths >= 32) & (offsets <= size)
    ok &= lengths <= size - np.minimum(offsets, size)
    ok &= c < snd.shape[0]
    idx = np.flatnonzero(ok)
    st = snd[c[idx].astype(np.int64)].astype(np.uint64)
    at = offsets[idx].astype(np.int64)
    seq = _be(arena, at + 16, 4)
    edge = ((arena[at + 25] & (SYN | FIN)) != 0).astype(np.uint64)
    una = st[:, 0]
    two32 = np.uint64(1 << 32)
    if rule == RULE_REF:
        owed = una < (seq + edge) % two32
    else:
        n_seq = _be(arena, at + 10, 2) + edge
        d = (seq + n_seq + two32 - una) % two32  # the i32 view of this is > 0 iff 0 < d < 2^31
        owed = (n_seq > 0) & (d > 0) & (d < np.uint64(1 << 31))
    keep = np.zeros(n, bool)
    keep[idx] = owed & ((st[:, 2] & np.uint64(CLOSED)) == 0)
    return keep


def resend_np(arena, snd, count=None, stride=0, length=0, offsets=None, lengths=None, conn=None, cap=None,
              rule=RULE_REF, mode=0):
    """-> (keep u8[count], out_offsets u64[w], out_lengths u32[w], out_conn u32[w], src u32[w], total), w =
    min(total, cap); arena (uint8, writable) patched in place on the kept images."""
    if offsets is None:
        offsets = np.arange(count, dtype=np.uint64) * np.uint64(stride)
        lengths = np.full(count, length, np.uint32)
    offsets, lengths = np.asarray(offsets, np.uint64), np.asarray(lengths, np.uint32)
    n = offsets.size
    keep = keep_np(arena, snd, offsets, lengths, conn, rule)
    src = np.flatnonzero(keep).astype(np.uint32)
    c = np.zeros(n, np.uint32) if conn is None else np.asarray(conn, np.uint32)
    if src.size:
        acks = np.asarray(snd, np.uint32).reshape(-1, 4)[c[src], 1]
        resend_batch_np(arena, offsets[src].astype(np.int64), lengths[src].astype(np.int64), acks, mode)
    total = int(src.size)
    w = total if cap is None else min(total, cap)
    src = src[:w]
    return keep.astype(np.uint8), offsets[src], lengths[src], c[src], src, total


class ResendGolden:
    def __init__(self):
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "resend_golden.json")) as f:
            meta = json.load(f)
        self.blob = np.fromfile(os.path.join(here, meta["blob"]), dtype=np.uint8)
        assert self.blob.size == meta["blob_bytes"]
        self.cases = meta["cases"]

    def queue(self):
        """The whole fixture as one mixed queue: image k is case k's image before the pass, at its
        offset in the blob's `before` part, and belongs to connection k whose state is the case's.
        -> (arena, offsets, lengths, conn, snd)."""
        n = len(self.cases)
        offsets = np.asarray([c["off"] for c in self.cases], np.uint64)
        lengths = np.asarray([c["len"] for c in self.cases], np.uint32)
        end = int((offsets + lengths).max())
        snd = np.asarray([[c["snd_una"], c["rcv_nxt"], CLOSED if c["closed"] else 0, 0] for c in self.cases], np.uint32)
        return self.blob[:end].copy(), offsets, lengths, np.arange(n, dtype=np.uint32), snd

    def keep(self):
        return np.asarray([c["keep"] for c in self.cases], np.uint8)

    def after(self, case):
        """The 32 header bytes of a kept case after the reference's pass."""
        return self.blob[case["after_off"]:case["after_off"] + 32]


def make_queue(seed, count, n_conns, fixed=False, stride=96, flaws=False, mode=0, p_keep=0.5, bad_ids=False):
    """A seeded queue of `count` images with valid checksums in `mode`: random headers, seq numbers
    around their connection's snd_una (below, equal, above, across the wrap), SYN / FIN / plain flag
    bytes, TcpLength 0 or the payload size.  fixed: every image stride - 32 bytes (the whole slot below
    64) at k * stride (-> offsets None); else an offset list with gaps.  flaws: some images short, odd
    or out of the arena.  bad_ids: some ids NONE or >= n_conns.  -> dict(arena, offsets, lengths, conn,
    snd, stride, length, count)."""
    rng = np.random.default_rng(seed)
    snd = np.zeros((max(n_conns, 1), 4), np.uint32)
    snd[:, 0] = rng.integers(0, 1 << 32, snd.shape[0], dtype=np.uint64)
    edges = np.asarray([0xFFFFFFF0, 0, 5, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 1, 0xFFFFFFFE], np.uint32)
    edges = edges[: min(8, max(1, n_conns // 2))]  # half of a small table sits at the edges of the u32 range
    snd[: edges.size, 0] = edges
    snd[:, 1] = rng.integers(0, 1 << 32, snd.shape[0], dtype=np.uint64)
    snd[:, 2] = (rng.random(snd.shape[0]) < 0.1) * CLOSED if n_conns > 2 else 0
    snd[:, 3] = rng.integers(0, 1 << 32, snd.shape[0], dtype=np.uint64)  # reserved: not looked at
    conn = rng.integers(0, max(n_conns, 1), count, dtype=np.uint64).astype(np.uint32)
    if fixed:
        length = stride - 32 if stride >= 64 else stride
        lengths = np.full(count, length, np.uint32)
        offsets = np.arange(count, dtype=np.uint64) * np.uint64(stride)
        arena = rng.integers(0, 256, count * stride + 6, dtype=np.uint8)
    else:
        length = 0
        lengths = (32 + 2 * rng.integers(0, 40, count)).astype(np.uint32)
        gaps = 2 * rng.integers(0, 9, count)
        offsets = (np.cumsum(lengths + gaps) - lengths).astype(np.uint64)
        arena = rng.integers(0, 256, int(offsets[-1] + lengths[-1]) + 6 if count else 6, dtype=np.uint8)
    at = offsets.astype(np.int64)
    una = snd[conn % snd.shape[0], 0].astype(np.int64)
    above = rng.random(count) < p_keep
    delta = np.where(above, rng.integers(1, 3000, count), -rng.integers(0, 3000, count))
    delta[rng.random(count) < 0.15] = 0
    delta[rng.random(count) < 0.05] = -1
    seq = ((una + delta) % (1 << 32)).astype(np.uint32)
    arena[at[:, None] + np.arange(16, 20)] = seq.astype(">u4").view(np.uint8).reshape(-1, 4)
    arena[at + 25] = np.asarray([ACK, ACK, ACK, SYN, FIN | ACK, SYN | ACK, 0], np.uint8)[rng.integers(0, 7, count)]
    tcplen = np.where(rng.random(count) < 0.3, 0, lengths - 32).astype(np.uint16)
    arena[at[:, None] + np.arange(10, 12)] = tcplen.astype(">u2").view(np.uint8).reshape(-1, 2)
    fill_batch_np(arena, at, lengths, mode)
    if flaws and count:
        lengths = lengths.copy()
        offsets = offsets.copy()
        pick = rng.random(count)
        lengths[pick < 0.04] = 30
        lengths[(pick >= 0.04) & (pick < 0.08)] += 1
        offsets[(pick >= 0.08) & (pick < 0.12)] += 1
        offsets[(pick >= 0.12) & (pick < 0.16)] = arena.size - 20
        offsets[(pick >= 0.16) & (pick < 0.18)] = np.uint64(0xFFFFFFFFFFFFFFF0)
        lengths[(pick >= 0.18) & (pick < 0.20)] = 0xFFFFFFFE
    if bad_ids:
        bad = rng.random(count) < 0.2
        conn[bad] = np.asarray([NONE, n_conns, n_conns + 1, 0x80000000, NONE - 1], np.uint32)[rng.integers(0, 5, int(bad.sum()))]
    return dict(arena=arena, offsets=None if fixed else offsets, lengths=None if fixed else lengths, conn=conn,
                snd=snd[:n_conns], stride=stride if fixed else 0, length=length, count=count)


def interleaved_queue(seed, n_conns=3, seg=64, mode=0, wrap=False):
    """n_conns send streams cut by segment_np, their images interleaved round robin in one arena of
    32 + seg byte slots: the queue of the loop tests.  wrap: connection 0's sequence numbers pass 2^32
    on the way (under the reference's plain compare an image left behind a wrapped snd_una is owed for
    ever, so only the serial rule drains such a queue).  -> dict(arena, offsets, lengths, conn, seq0, seg,
    nseg)."""
    rng = np.random.default_rng(seed)
    stride = 32 + seg
    parts, nseg, seq0 = [], [], []
    for c in range(n_conns):
        pay = rng.integers(0, 256, seg * int(rng.integers(5, 12)) + 2 * int(rng.integers(0, seg // 2)), dtype=np.uint8)
        hdr = rng.integers(0, 256, 32, dtype=np.uint8)
        hdr[25] = ACK
        s0 = 0xFFFFFFFF - 3 * seg if wrap and c == 0 else int(rng.integers(0, 1 << 31))
        imgs, lens, _ = segment_np(pay, seg, hdr, s0, stride=stride, mode=mode)
        parts.append((imgs, lens))
        nseg.append(lens.size)
        seq0.append(s0)
    order = [(k, c) for c in range(n_conns) for k in range(nseg[c])]
    order.sort(key=lambda kc: (kc[0], kc[1]))  # round robin: per connection in stream order
    arena = np.zeros(len(order) * stride, np.uint8)
    offsets, lengths, conn = [], [], []
    for slot, (k, c) in enumerate(order):
        imgs, lens = parts[c]
        arena[slot * stride:slot * stride + stride] = imgs[k * stride:(k + 1) * stride]
        offsets.append(slot * stride)
        lengths.append(int(lens[k]))
        conn.append(c)
    return dict(arena=arena, offsets=np.asarray(offsets, np.uint64), lengths=np.asarray(lengths, np.uint32),
                conn=np.asarray(conn, np.uint32), seq0=seq0, seg=seg, nseg=nseg)
