"""numpy restatement of the batched reply builder, for the tests.

reply_np:    tcpck_batch_reply / tcpck_build_replies (include/tcpck.h) -- the
             planners' verdicts to the dense ring of 32-B ACK / RST datagrams the
             reference sends back (SendAck, socket-internal.h:293-299; the RST of a
             datagram of no socket, socket-manager.h:201-207), vectorised.
ReplyGolden: tests/golden/reply_golden.{bin,json}: those datagrams built by the
             reference's own inline helpers (tests/golden/gen_reply.cc).
"""
import json
import os

import numpy as np

SEND_ACK, RST, HOST = 4, 16, 32
NONE = 0xFFFFFFFF
MODE_REF, MODE_RFC1071 = 0, 1


def checksums_np(images, mode):
    """The checksum of each 32-B row (bytes 28-29 taken as zero): ~ of the sum of the sixteen
    little-endian u16 words, mod 2^16 (REF, tcp-header.h:252-263) or with the carries folded
    back in (RFC 1071)."""
    w = images.reshape(-1, 16, 2).astype(np.uint32)
    words = w[:, :, 0] | (w[:, :, 1] << 8)
    words[:, 14] = 0
    s = words.sum(axis=1)  # at most 16 * 0xFFFF
    if mode == MODE_RFC1071:
        s = (s & 0xFFFF) + (s >> 16)
        s = (s & 0xFFFF) + (s >> 16)
    return (~s & 0xFFFF).astype(np.uint16)


def be32(values):
    """u32 array -> (n, 4) bytes, network order."""
    return np.asarray(values, np.uint32).astype(">u4").view(np.uint8).reshape(-1, 4)


def reply_np(verdict, ack, conn, tmpl, n_conns, cap, mode):
    """-> (replies u8[min(total, cap), 32], src u32[min(total, cap)], total).  conn None: every
    image is connection 0.  tmpl: at least 32 * n_conns bytes."""
    verdict = np.asarray(verdict, np.uint8)
    ack = np.asarray(ack, np.uint32)
    n = verdict.size
    c = np.zeros(n, np.uint32) if conn is None else np.asarray(conn, np.uint32)
    is_rst = (verdict & RST) != 0
    is_ack = ~is_rst & ((verdict & SEND_ACK) != 0) & (c < n_conns)
    src = np.flatnonzero(is_rst | is_ack).astype(np.uint32)
    total = int(src.size)
    src = src[:cap]
    rows = np.zeros((src.size, 32), np.uint8)
    a = is_ack[src]
    if a.any():
        t = np.asarray(tmpl, np.uint8).reshape(-1)[:32 * n_conns].reshape(n_conns, 32)
        rows[a] = t[c[src[a]]]
        rows[a, 20:24] = be32(ack[src[a]])
        rows[a, 25] |= 0x08
    r = ~a
    rows[r, 16:20] = be32(ack[src[r]])
    rows[r, 25] = 0x20
    rows[:, 28:30] = checksums_np(rows, mode).astype("<u2").view(np.uint8).reshape(-1, 2)
    return rows, src, total


def template_np(seq, wnd, src_ip=0, src_port=0, dst_ip=0, dst_port=0):
    """A connection's 32-B network-order template, zero outside the fields SetSource,
    SetDestination and AckHeader's seq / window set."""
    t = np.zeros(32, np.uint8)
    t[0:4] = be32([src_ip])[0]
    t[4:8] = be32([dst_ip])[0]
    t[12:14] = [src_port >> 8, src_port & 0xFF]
    t[14:16] = [dst_port >> 8, dst_port & 0xFF]
    t[16:20] = be32([seq])[0]
    t[26:28] = [wnd >> 8, wnd & 0xFF]
    return t


class ReplyGolden:
    def __init__(self):
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "reply_golden.json")) as f:
            meta = json.load(f)
        self.blob = np.fromfile(os.path.join(here, meta["blob"]), dtype=np.uint8)
        assert self.blob.size == meta["blob_bytes"] == 32 * len(meta["cases"])
        self.cases = meta["cases"]
        self.images = self.blob.reshape(-1, 32)

    def ring(self):
        """The whole fixture as one ring: image k belongs to connection k, whose template is case
        k's; the verdict is what the planners give such an image (ACCEPT | PAYLOAD | SEND_ACK, BAD_SUM
        | SEND_ACK, or RST), the ack number the case's.  -> (verdict, ack, conn, tmpl)."""
        n = len(self.cases)
        verdict = np.asarray([RST if c["kind"] == "rst" else (7, 12)[k % 2] for k, c in enumerate(self.cases)], np.uint8)
        ack = np.asarray([c["ack"] for c in self.cases], np.uint32)
        tmpl = np.concatenate([template_np(c["seq"], c["wnd"], c["src_ip"], c["src_port"], c["dst_ip"], c["dst_port"])
                               for c in self.cases])
        return verdict, ack, np.arange(n, dtype=np.uint32), tmpl

    def rfc_images(self, fill16):
        """The REF images with the checksum cleared and refilled by tcpck_fill16 in RFC 1071 mode
        (the reference has no such mode)."""
        out = self.images.copy()
        for row in out:
            fill16(row, MODE_RFC1071)
        return out


def random_ring(seed, count, n_conns, p_reply=0.5, p_rst=0.1, bad_ids=False):
    """A seeded ring: verdict bytes as the planners write them (ACCEPT 1, PAYLOAD 2, SEND_ACK 4,
    BAD_SUM 8, RST 16, HOST 32, and 0), ack numbers, connection ids, random templates.  bad_ids: some
    ids are NONE or >= n_conns."""
    rng = np.random.default_rng(seed)
    replying = rng.random(count) < p_reply
    rst = rng.random(count) < p_rst
    silent = np.asarray([0, 1, 3, HOST, 8], np.uint8)[rng.integers(0, 5, count)]
    acks = np.asarray([7, 5, 12, 4], np.uint8)[rng.integers(0, 4, count)]
    verdict = np.where(replying, np.where(rst, np.uint8(RST), acks), silent).astype(np.uint8)
    ack = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    conn = rng.integers(0, max(n_conns, 1), count, dtype=np.uint64).astype(np.uint32)
    if bad_ids:
        bad = rng.random(count) < 0.2
        conn[bad] = np.asarray([NONE, n_conns, n_conns + 1, 0x80000000], np.uint32)[rng.integers(0, 4, int(bad.sum()))]
    tmpl = rng.integers(0, 256, 32 * n_conns, dtype=np.uint8)
    return verdict, ack, conn, tmpl
