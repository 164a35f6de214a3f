"""The receive path in a closed loop: rings in sequence against a sender model.

A seeded Scenario holds connections with send streams; a go-back-N sender
(Loop) offers up to W images of each connection per ring, perturbed (drop,
duplicate, swap, a damaged copy), rewrites their acknowledgement numbers by the
resend path, and advances only on what it reads out of the reply ring's BYTES.
The receiver's half of a ring -- receive, demux, plan on a persistent
tcpck_conn_state array, deliver into one shared buffer, reply -- is a backend:

  NumpyBackend   receive_np, demux_np over a dict, plan_multi_np over persistent
                 dicts, deliver_np on a shadow buffer, reply_np;
  LibTwin        the library's host calls on the numpy backend's inputs
                 (tcpck.plan_deliver_multi, tcpck.build_replies, a host-only
                 ConnTable), tests/test_ring_loop.py;
  DeviceBackend  the C ABI's device calls on one stream, every buffer allocated
                 once, tests/test_gpu_ring_loop.py.

The end-to-end oracle needs no restatement: every connection's receive stream
must end up equal to its send stream.  No pytest in here.
"""
import contextlib

import numpy as np

from deliver_np import ACCEPT, F_ACK, F_FIN, F_SYN, SKIP, deliver_np, header_fields
from demux_np import CONN_HOST, HOST, NOT_STOPPED, STATE_KEYS, demux_np, interleave, plan_multi_np
from oracle.ref16 import fill_np, receive_np, resend_batch_np, segment_np
from reply_np import reply_np, template_np

M32 = 0xFFFFFFFF
SENTINEL = 0xA5   # the shared receive buffer, the reply ring and the scratch guard before the first ring
UNSET = 0xEE      # d_ok, d_hdr, d_conn before the first ring
W = 120           # images a connection offers per ring
MAX_RING = 1536   # the fixed size of every per-image device array
SPARE_SLOTS = 40  # damaged copies a ring can hold
SPARE_STRIDE = 9040
EXTRA_STRIDE = 160
P_DROP = P_DUP = P_DAMAGE = P_SWAP = 0.02
P_BAD_ACK = 0.004  # ack = snd_nxt + 1: the reference's plain `ack <= snd_nxt` rejects it (state.cc:198)
ACK_STEPS = 24     # the sender's ack number reaches the receiver's snd_nxt after this many rings
SYN_RINGS = (1, 3)
LATE_SET_RING, ERASE_RING, REMAP_RING = 2, 3, 4
RST_RINGS_BEFORE_ABORT = 2  # the erased connection's peer gives up after RSTs in this many rings
HARD_STOP = 200    # only keeps a broken loop from spinning: reaching it is a failure
HOST_IP = 0x7F000001
LISTEN_PORT = 7000
FIELDS = STATE_KEYS + ("recv_base", "recv_bytes", "stopped_at", "flags")

# rings until every connection in the table has its data acknowledged, measured on the numpy
# backend (the loop is deterministic; both modes give the same count): {(seed, plain): rings}
RING_COUNT = {(0, 2): 24, (1, 2): 26, (2, 3): 19}


def _be32(row, at):
    return int(row[at]) << 24 | int(row[at + 1]) << 16 | int(row[at + 2]) << 8 | int(row[at + 3])


class Scenario:
    """Everything that is fixed before ring 0: the connections, the arena's and the shared
    receive buffer's layout, the datagrams of the peers without a table entry."""

    ROLES = ("wrap32", "wrap32_tiny", "cross31", "small_window", "fin", "late", "erased", "remap")

    def __init__(self, seed, mode=0, plain=2):
        rng = np.random.default_rng([seed, 0x5EED])
        self.seed, self.mode, self.rings = seed, mode, RING_COUNT.get((seed, plain))
        roles = self.ROLES + ("plain",) * plain
        segs = (1460, 4, 9000, 536, 100, 100, 536, 1460) + tuple((4, 100, 1460)[i % 3] for i in range(plain))
        self.conns, at, recv_at = [], 0, 6
        for c, (role, seg) in enumerate(zip(roles, segs)):
            n_img = {"cross31": int(rng.integers(130, 150)), "small_window": 140, "fin": 130, "erased": 200}.get(
                role, int(rng.integers(150, 260 if seg <= 100 else 220)))
            last = 2 if seg == 4 else 2 * int(rng.integers(1, seg // 2))
            P = (n_img - 1) * seg + last
            iss = {"wrap32": (1 << 32) - P // 2, "wrap32_tiny": (1 << 32) - 301,
                   "cross31": (1 << 31) - P // 3}.get(role, int(rng.integers(1, 1 << 30)))
            snd_nxt = 0xFFFFFFFE if role == "cross31" else int(rng.integers(1 << 28, 1 << 32) - 2)
            step = 1 if c == 0 else int(rng.integers(1, 1 << 22))
            n_data = n_img - 1 if role == "fin" else n_img  # (the FIN image's payload is never appended)
            data_bytes = P - last if role == "fin" else P
            recv_bytes = 10 * seg + 2 if role == "small_window" else data_bytes
            stride = (32 + seg + 15) // 16 * 16
            cn = dict(role=role, seg=seg, n_img=n_img, n_data=n_data, P=P, data_bytes=data_bytes, iss=iss,
                      stream=rng.integers(0, 256, P, dtype=np.uint8), host_port=8000 + c,
                      peer_ip=0x0A000001 + 257 * c, peer_port=40000 + 3 * c, snd_nxt=snd_nxt,
                      snd_una0=snd_nxt - ACK_STEPS * step, step=step, base=at, stride=stride,
                      recv_base=recv_at, recv_bytes=recv_bytes)
            if role == "plain" and c == len(self.ROLES):  # the erased connection's neighbour: only the peer port differs
                cn.update(host_port=self.conns[6]["host_port"], peer_ip=self.conns[6]["peer_ip"])
            lens = np.full(n_img, 32 + seg, np.uint32)
            lens[-1] = 32 + last
            cn["lens"] = lens
            cn["send_tmpl"] = template_np(0, 512 + c, cn["peer_ip"], cn["peer_port"], HOST_IP, cn["host_port"])
            cn["send_tmpl"][20:24] = np.frombuffer(int(cn["snd_una0"]).to_bytes(4, "big"), np.uint8)
            cn["send_tmpl"][25] = F_ACK
            cn["reply_tmpl"] = template_np(snd_nxt, 1024 + c, HOST_IP, cn["host_port"], cn["peer_ip"], cn["peer_port"])
            cn["reply_tmpl"][9] = 6
            self.conns.append(cn)
            at += n_img * stride
            recv_at += recv_bytes + 2 * int(rng.integers(1, 20))
        self.n_conns = len(self.conns)
        self.listener, self.remap_to, self.n_states = self.n_conns, self.n_conns + 1, self.n_conns + 2
        self.recv_total = recv_at
        self.poison_tmpl = template_np(0, 0, 0, 1, 0, 1)  # ports (1, 1): no connection's
        # the peers without a table entry, and the SYN to the listener
        self.extras, self.extra_base = [], at
        blob = []
        peers = ((0xC0A80001, 50001), (0xC0A80002, 50002))
        for j in range(13):
            ip, port = peers[j % 2]
            syn = j == 12
            pay = (0, 2, 100)[j % 3]
            img = np.zeros(EXTRA_STRIDE, np.uint8)
            ack = int(rng.integers(0, 1 << 32))
            dport = LISTEN_PORT if syn or j % 4 == 0 else (self.conns[j % 3]["host_port"] if j % 4 == 1 else 9000 + j)
            img[:32] = template_np(int(rng.integers(0, 1 << 32)), 77, ip, port, HOST_IP, dport)
            img[10:12] = (pay >> 8, pay & 0xFF)
            img[20:24] = np.frombuffer(ack.to_bytes(4, "big"), np.uint8)
            img[25] = F_SYN if syn else F_ACK
            img[32:32 + pay] = rng.integers(0, 256, pay, dtype=np.uint8)
            fill_np(img[:32 + pay], mode)
            bad = not syn and j % 3 == 2 and j % 2 == 1 or j == 8
            if bad:
                img[int(rng.integers(0, 32 + pay))] ^= 1 << int(rng.integers(0, 8))
            self.extras.append(dict(off=at, len=32 + pay, ack=ack, syn=syn, bad=bool(bad)))
            blob.append(img)
            at += EXTRA_STRIDE
        self.extra_bytes = np.concatenate(blob)
        self.spare_base = at
        self.arena_bytes = at + SPARE_SLOTS * SPARE_STRIDE

    def ack_at(self, c, ring):
        """The acknowledgement number connection c's sender writes in ring `ring`."""
        cn = self.conns[c]
        return min(cn["snd_una0"] + cn["step"] * (ring + 1), cn["snd_nxt"])

    def initial_state(self, i):
        if i < self.n_conns:
            cn = self.conns[i]
            return dict(rcv_nxt=cn["iss"] & M32, snd_nxt=cn["snd_nxt"], snd_una=cn["snd_una0"], rcv_wnd=0, delivered=0,
                        recv_base=cn["recv_base"], recv_bytes=cn["recv_bytes"], stopped_at=NOT_STOPPED, flags=0)
        return dict(rcv_nxt=0x1234 if i == self.listener else 0, snd_nxt=0, snd_una=0, rcv_wnd=0, delivered=0,
                    recv_base=0, recv_bytes=0, stopped_at=NOT_STOPPED, flags=CONN_HOST if i == self.listener else 0)

    def initial_templates(self):
        t = np.tile(self.poison_tmpl, self.n_states)
        for c, cn in enumerate(self.conns):
            t[32 * c:32 * c + 32] = cn["reply_tmpl"]
        return t

    def fin_header(self, arena, update16=None):
        """The FIN connection's last image with FIN set and the checksum put right: by the full
        recompute (update16 None) or by `update16` on the one word that changed."""
        cn = self.conns[4]
        off = cn["base"] + (cn["n_img"] - 1) * cn["stride"]
        ln = int(cn["lens"][-1])
        img = arena[off:off + ln].copy()
        old = int(img[24]) | int(img[25]) << 8
        img[25] |= F_FIN
        if update16 is None:
            fill_np(img, self.mode)
        else:
            cs = update16(int(img[28]) | int(img[29]) << 8, old, int(img[24]) | int(img[25]) << 8, self.mode)
            img[28], img[29] = cs & 0xFF, cs >> 8
        return off, img[:32]


class Ring:
    """One ring as the sender made it: the arrival order (offsets, lengths), the ACK rewrite that
    precedes it (rw_*: unique offsets), the damaged copies taken after the rewrite, and what the
    sender knows of every image (owner: connection or -1, idx: image index within it or the
    extra's number, ack: the acknowledgement number it carries)."""


class Backend:
    """What the loop asks of a receiver.  States are dicts of FIELDS on this interface."""

    def start(self, scn, mode):
        self.scn, self.mode = scn, mode
        self.log = [bytearray() for _ in scn.conns]  # the application's reads of drained windows

    def move_state(self, a, b):
        self.put_state(b, self.get_state(a))

    def set_flags(self, i, flags):
        st = self.get_state(i)
        st["flags"] = flags
        self.put_state(i, st)

    def drain(self, c, i):
        """The application consumes connection c's window (state i): its delivered bytes go to the
        log, rcv.delivered restarts at the window's front."""
        st = self.get_state(i)
        self.log[c] += self.recv_host()[st["recv_base"]:st["recv_base"] + st["delivered"]].tobytes()
        st["delivered"] = 0
        self.put_state(i, st)

    def states(self):
        return [tuple(self.get_state(i)[f] for f in FIELDS) for i in range(self.scn.n_states)]


class NumpyBackend(Backend):
    def __init__(self, scn, mode):
        self.start(scn, mode)
        self.table, self.st = {}, [scn.initial_state(i) for i in range(scn.n_states)]
        self.tmpl = scn.initial_templates()
        self.arena = np.zeros(scn.arena_bytes, np.uint8)
        for cn in scn.conns:
            imgs, lens, _ = segment_np(cn["stream"], cn["seg"], cn["send_tmpl"], cn["iss"] & M32, cn["stride"], mode)
            assert np.array_equal(lens, cn["lens"])
            self.arena[cn["base"]:cn["base"] + imgs.size] = imgs
        self.arena[scn.extra_base:scn.extra_base + scn.extra_bytes.size] = scn.extra_bytes
        self.recv = np.full(scn.recv_total, SENTINEL, np.uint8)
        self.ok = np.full(MAX_RING, UNSET, np.uint8)
        self.hdr = np.full(32 * MAX_RING, UNSET, np.uint8)
        self.conn = np.full(MAX_RING, UNSET * 0x01010101, np.uint32)
        self.replies = np.full(32 * (MAX_RING + 2), SENTINEL, np.uint8)
        self.src = np.full(MAX_RING + 2, M32, np.uint32)

    def arena_host(self):
        return self.arena

    def set_fin(self):
        off, h = self.scn.fin_header(self.arena)
        self.arena[off:off + 32] = h

    def recv_host(self):
        return self.recv

    def table_set(self, key, i):
        self.table[key] = i

    def table_erase(self, key):
        self.table.pop(key, None)

    def table_commit(self):
        pass

    def get_state(self, i):
        return dict(self.st[i])

    def put_state(self, i, st):
        self.st[i].update(st)

    def set_template(self, i, t):
        self.tmpl[32 * i:32 * i + 32] = t

    def ring(self, R):
        n, a = R.n, self.arena
        if R.rw_off.size:
            resend_batch_np(a, R.rw_off, R.rw_len, R.rw_ack, self.mode)
        for s, d, ln, pos, bit in R.damage:
            a[d:d + ln] = a[s:s + ln]
            a[d + pos] ^= 1 << bit
        wire = a.copy()
        off = R.offsets.astype(np.int64)
        self.ok[:n] = receive_np(wire, off, R.lengths, self.mode)
        self.hdr[:32 * n] = wire[off[:, None] + np.arange(32)[None, :]].reshape(-1)
        self.conn[:n] = demux_np(self.hdr[:32 * n], self.table)
        dst, verdict, ack = plan_multi_np(self.hdr[:32 * n], self.ok[:n], self.conn[:n], R.lengths, self.st)
        deliver_np(a, R.offsets, R.lengths, dst, self.recv)
        rows, src, total = reply_np(verdict, ack, self.conn[:n], self.tmpl, self.scn.n_states, MAX_RING, self.mode)
        self.replies[:rows.size] = rows.reshape(-1)
        self.src[:src.size] = src
        return dict(arena=a.copy(), ok=self.ok.copy(), hdr=self.hdr.copy(), conn=self.conn.copy(), dst=dst, verdict=verdict,
                    ack=ack, recv=self.recv.copy(), replies=self.replies.copy(), src=self.src.copy(),
                    count=np.asarray([total, -1], np.int64), guard=np.full(64, SENTINEL, np.uint8), states=self.states())


class CStates(Backend):
    """A backend whose states are a tcpck.ConnState array (self.cs)."""

    def make_states(self):
        import tcpck
        self.cs = (tcpck.ConnState * self.scn.n_states)()
        for i in range(self.scn.n_states):
            self.put_state(i, self.scn.initial_state(i))

    def get_state(self, i):
        s = self.cs[i]
        d = {k: getattr(s.rcv, k) for k in STATE_KEYS}
        d.update(recv_base=s.recv_base, recv_bytes=s.recv_bytes, stopped_at=s.stopped_at, flags=s.flags)
        return d

    def put_state(self, i, st):
        s = self.cs[i]
        for k in STATE_KEYS:
            setattr(s.rcv, k, st[k])
        s.recv_base, s.recv_bytes, s.stopped_at, s.flags = st["recv_base"], st["recv_bytes"], st["stopped_at"], st["flags"]


class LibTwin(CStates):
    """The library's host twins beside the numpy backend: a host-only ConnTable, tcpck.
    plan_deliver_multi on a persistent ConnState array, tcpck.build_replies -- on the numpy
    backend's ok / hdr / conn of the same ring."""

    def __init__(self, scn, mode):
        import tcpck
        self.start(scn, mode)
        self.tcpck = tcpck
        self.make_states()
        self.table = tcpck.ConnTable(None, 64)
        self.tmpl = scn.initial_templates()

    def table_set(self, key, i):
        self.table.set(*key, i)

    def table_erase(self, key):
        self.table.erase(*key)

    def table_commit(self):
        self.table.commit()

    def set_template(self, i, t):
        self.tmpl[32 * i:32 * i + 32] = t

    def drain(self, c, i):
        self.cs[i].rcv.delivered = 0

    def ring(self, R, np_out):
        n = R.n
        ok, hdr, conn = np_out["ok"][:n], np_out["hdr"][:32 * n], np_out["conn"][:n]
        dst, verdict, ack = self.tcpck.plan_deliver_multi(hdr, ok, conn, self.cs, lengths=R.lengths)
        rows, src, total = self.tcpck.build_replies(verdict, ack, self.tmpl, conn=conn, reply_cap=MAX_RING, mode=self.mode)
        return dict(dst=dst, verdict=verdict, ack=ack, rows=rows, src=src, total=total, states=self.states())


class DeviceBackend(CStates):
    """The receive path's device calls through the C ABI, every one on `stream` (a
    torch.cuda.Stream; None: the null stream).  Every device and pinned buffer is allocated here,
    once; a ring synchronises twice: after the copy down the planner needs, and after the
    read-back the comparisons need.  ring_steps() yields after every enqueued call, so two loops
    can be interleaved call by call."""

    def __init__(self, scn, mode, ctx, stream=None):
        import tcpck
        import torch
        self.start(scn, mode)
        self.tcpck, self.torch, self.ctx, self.ts = tcpck, torch, ctx, stream
        self.make_states()
        dev = lambda n, dt, fill: torch.full((n,), fill, dtype=dt, device="cuda")
        pin = lambda n, dt: torch.zeros(n, dtype=dt).pin_memory()
        with self._on():
            self.d_arena = dev(scn.arena_bytes, torch.uint8, 0)
            for cn in scn.conns:
                d_pay = torch.from_numpy(cn["stream"]).cuda()
                n = ctx.batch_segment(d_pay, cn["P"], cn["seg"], cn["send_tmpl"], cn["iss"] & M32,
                                      self.d_arena[cn["base"]:], cn["stride"], mode=mode, stream=stream)
                assert n == cn["n_img"]
                self._sync()  # (d_pay goes out of use here)
            self.d_arena[scn.extra_base:scn.extra_base + scn.extra_bytes.size].copy_(torch.from_numpy(scn.extra_bytes))
            self.d_off, self.h_off = dev(MAX_RING, torch.int64, 0), pin(MAX_RING, torch.int64)
            self.d_len, self.h_len = dev(MAX_RING, torch.int32, 0), pin(MAX_RING, torch.int32)
            self.d_rw_off, self.h_rw_off = dev(MAX_RING, torch.int64, 0), pin(MAX_RING, torch.int64)
            self.d_rw_ack, self.h_rw_ack = dev(MAX_RING, torch.int32, 0), pin(MAX_RING, torch.int32)
            self.d_ok, self.h_ok = dev(MAX_RING, torch.uint8, UNSET), pin(MAX_RING, torch.uint8)
            self.d_hdr, self.h_hdr = dev(32 * MAX_RING, torch.uint8, UNSET), pin(32 * MAX_RING, torch.uint8)
            self.d_conn, self.h_conn = dev(MAX_RING, torch.int32, 0), pin(MAX_RING, torch.int32)
            self.d_conn.view(torch.uint8).fill_(UNSET)
            self.d_dst, self.h_dst = dev(MAX_RING, torch.int64, -1), pin(MAX_RING, torch.int64)
            self.d_verdict, self.h_verdict = dev(MAX_RING, torch.uint8, 0), pin(MAX_RING, torch.uint8)
            self.d_ack, self.h_ack = dev(MAX_RING, torch.int32, 0), pin(MAX_RING, torch.int32)
            self.d_recv, self.h_recv = dev(scn.recv_total, torch.uint8, SENTINEL), pin(scn.recv_total, torch.uint8)
            self.d_rep, self.h_rep = dev(32 * (MAX_RING + 2), torch.uint8, SENTINEL), pin(32 * (MAX_RING + 2), torch.uint8)
            self.d_src, self.h_src = dev(MAX_RING + 2, torch.int32, -1), pin(MAX_RING + 2, torch.int32)
            self.d_cnt, self.h_cnt = dev(2, torch.int64, -1), pin(2, torch.int64)
            self.scr_bytes = tcpck.reply_scratch_bytes(MAX_RING)
            self.d_scr, self.h_guard = dev(self.scr_bytes + 64, torch.uint8, SENTINEL), pin(64, torch.uint8)
            self.h_arena = pin(scn.arena_bytes, torch.uint8)
            self.d_tmpl = torch.from_numpy(scn.initial_templates()).cuda()
            self.h_recv.copy_(self.d_recv)
        self._sync()
        self.table = tcpck.ConnTable(ctx, 64)
        self.graph = None

    def close(self):
        self.graph = None
        self.table.close()

    def _on(self):
        return self.torch.cuda.stream(self.ts) if self.ts is not None else contextlib.nullcontext()

    def _sync(self):
        (self.ts if self.ts is not None else self.torch.cuda.current_stream()).synchronize()

    def _up(self, h, d, x):
        """Host array -> device through the pinned twin, in stream order, no synchronisation."""
        k = x.size
        h[:k].copy_(self.torch.from_numpy(x))
        with self._on():
            d[:k].copy_(h[:k], non_blocking=True)

    def _down(self, pairs):
        with self._on():
            for h, d in pairs:
                h.copy_(d[:h.numel()] if d.numel() != h.numel() else d, non_blocking=True)

    def arena_host(self):
        self._down([(self.h_arena, self.d_arena)])
        self._sync()
        return self.h_arena.numpy().copy()

    def set_fin(self):
        """Control plane, before ring 0: the FIN bit by tcpck_update16 on the stored checksum."""
        off, h = self.scn.fin_header(self.arena_host(), self.tcpck.update16)
        with self._on():
            self.d_arena[off:off + 32].copy_(self.torch.from_numpy(h))
        self._sync()

    def recv_host(self):
        return self.h_recv.numpy()  # as the last ring's read-back left it

    def table_set(self, key, i):
        self.table.set(*key, i)

    def table_erase(self, key):
        self.table.erase(*key)

    def table_commit(self):
        self.table.commit(stream=self.ts)

    def set_template(self, i, t):
        with self._on():
            self.d_tmpl[32 * i:32 * i + 32].copy_(self.torch.from_numpy(np.ascontiguousarray(t)))
        self._sync()

    def _second_half(self, count):
        self.ctx.batch_deliver(self.d_arena, count, self.d_dst, self.d_recv, self.scn.recv_total, offsets=self.d_off,
                               lengths=self.d_len, stream=self.ts)
        self.ctx.batch_reply(self.d_verdict, self.d_ack, self.d_tmpl, self.scn.n_states, count, self.d_rep, MAX_RING,
                             self.d_cnt, self.d_scr, conn=self.d_conn, src=self.d_src, mode=self.mode, stream=self.ts)

    def capture(self, count):
        """batch_deliver + batch_reply over `count` images of the fixed device buffers, captured on
        this backend's one stream (a linear chain) into a graph that every later ring replays."""
        assert self.ts is not None and count <= MAX_RING
        g = self.torch.cuda.CUDAGraph()
        with self.torch.cuda.stream(self.ts):
            with self.torch.cuda.graph(g, stream=self.ts):
                self._second_half(count)
        self.graph, self.graph_count = g, count

    def ring_steps(self, R):
        n, m, s, ctx = R.n, R.rw_off.size, self.ts, self.ctx
        # the sender: the resend path over the ring's unique images, then the damaged copies
        if m:
            self._up(self.h_rw_off, self.d_rw_off, R.rw_off.view(np.int64))
            self._up(self.h_rw_ack, self.d_rw_ack, R.rw_ack.view(np.int32))
            ctx.batch_set_ack(self.d_arena, m, acks=self.d_rw_ack, offsets=self.d_rw_off, mode=self.mode, stream=s)
            yield
        with self._on():
            for src, dst, ln, pos, bit in R.damage:
                self.d_arena[dst:dst + ln].copy_(self.d_arena[src:src + ln])
                self.d_arena[dst + pos:dst + pos + 1].bitwise_xor_(1 << bit)
        yield
        # the receiver
        N = n if self.graph is None else self.graph_count  # a captured second half runs on N images: the rest padding
        assert n <= N
        pad = lambda x, fill: x if N == n else np.concatenate([x, np.full(N - n, fill, x.dtype)])
        self._up(self.h_off, self.d_off, pad(R.offsets, 0).view(np.int64))
        self._up(self.h_len, self.d_len, pad(R.lengths, 32).view(np.int32))
        ctx.batch_receive(self.d_arena, n, self.d_ok, self.d_hdr, offsets=self.d_off, lengths=self.d_len, mode=self.mode,
                          stream=s)
        yield
        ctx.batch_demux(self.table, self.d_hdr, n, self.d_conn, stream=s)
        yield
        self._down([(self.h_ok, self.d_ok), (self.h_hdr, self.d_hdr), (self.h_conn, self.d_conn)])
        self._sync()  # the copy down
        ok, hdr = self.h_ok.numpy().copy(), self.h_hdr.numpy().copy()
        conn = self.h_conn.numpy().view(np.uint32).copy()
        dst, verdict, ack = self.tcpck.plan_deliver_multi(hdr[:32 * n], ok[:n], conn[:n], self.cs, lengths=R.lengths)
        self._up(self.h_dst, self.d_dst, pad(dst, SKIP).view(np.int64))  # the copy up
        self._up(self.h_verdict, self.d_verdict, pad(verdict, 0))
        self._up(self.h_ack, self.d_ack, pad(ack, 0).view(np.int32))
        yield
        if self.graph is None:
            self._second_half(n)
            yield
        else:
            with self._on():
                self.graph.replay()
            yield
        self._down([(self.h_arena, self.d_arena), (self.h_recv, self.d_recv), (self.h_rep, self.d_rep),
                    (self.h_src, self.d_src), (self.h_cnt, self.d_cnt), (self.h_guard, self.d_scr[self.scr_bytes:])])
        self._sync()  # the read-back
        self.out = dict(arena=self.h_arena.numpy().copy(), ok=ok, hdr=hdr, conn=conn, dst=dst, verdict=verdict, ack=ack,
                        recv=self.h_recv.numpy().copy(), replies=self.h_rep.numpy().copy(),
                        src=self.h_src.numpy().view(np.uint32).copy(), count=self.h_cnt.numpy().copy(),
                        guard=self.h_guard.numpy().copy(), states=self.states())

    def ring(self, R):
        for _ in self.ring_steps(R):
            pass
        return self.out


WHOLE = ("arena", "ok", "hdr", "conn", "dst", "verdict", "ack", "recv", "replies", "src", "count", "guard")


def compare(ring, got, want, keys=WHOLE):
    """Whole arrays of one ring, two backends."""
    for k in keys:
        if not np.array_equal(got[k], want[k]):
            at = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8] if got[k].shape == want[k].shape else None
            raise AssertionError(f"ring {ring}: {k} differs at {at}")
    assert got["states"] == want["states"], (ring, [(i, a, b) for i, (a, b) in
                                                    enumerate(zip(got["states"], want["states"])) if a != b])


class Loop:
    """The sender, the control plane and the application around a list of backends that advance
    on identical rings; the sender reads the FIRST backend's reply bytes."""

    def __init__(self, scn, backends):
        self.scn, self.backends, self.r = scn, backends, 0
        self.rng = np.random.default_rng([scn.seed, 0x100B])
        n = scn.n_conns
        self.una = [0] * n               # first unacknowledged image per connection
        self.cid = list(range(n))        # the id the table holds for each connection
        self.in_table = set()
        self.erased = None               # (connection, its window, its state) when it was erased
        self.aborted = set()
        self.rst_rings = [0] * n
        self.by_ports = {(cn["host_port"], cn["peer_port"]): c for c, cn in enumerate(scn.conns)}
        self.rewrites = {}
        self.sizes = []
        self.drained_last = False
        self.fin_host = False
        self.cov = dict(dropped=[0] * n, duplicated=[0] * n, swapped=[0] * n, damaged=[0] * n, full_drains=0, resumed=0,
                        fin_stops=0, fin_host=0, listener_host=0, unknown_host=0, unknown_rst=0, rst_before_set=0,
                        rst_after_erase=0, bad_ack_rejected=0)

    # ---- before ring 0
    def start(self):
        ref = self.backends[0].arena_host()
        for b in self.backends[1:]:
            if hasattr(b, "arena_host"):
                assert np.array_equal(b.arena_host(), ref), "the segmented arenas differ before the first ring"
        for b in self.backends:
            if hasattr(b, "set_fin"):
                b.set_fin()

    def key(self, c):
        cn = self.scn.conns[c]
        return cn["host_port"], cn["peer_ip"], cn["peer_port"]

    def each(self, f, *a):
        for b in self.backends:
            getattr(b, f)(*a)

    # ---- the control plane, between rings
    def control(self):
        scn, r = self.scn, self.r
        steps = []
        if r == 0:
            for c, cn in enumerate(scn.conns):
                if cn["role"] != "late":
                    self.each("table_set", self.key(c), c)
                    self.in_table.add(c)
            self.each("table_set", (LISTEN_PORT, 0, 0), scn.listener)
            steps.append("set")
        if r == LATE_SET_RING:
            self.each("table_set", self.key(5), 5)
            self.in_table.add(5)
            steps.append("late set")
        if r == ERASE_RING:
            b = self.backends[0]
            st = b.get_state(6)
            self.erased = (6, b.recv_host()[st["recv_base"]:st["recv_base"] + st["recv_bytes"]].copy(), st)
            self.each("table_erase", self.key(6))
            self.in_table.discard(6)
            steps.append("erase")
        if r == REMAP_RING:
            self.each("table_set", self.key(7), scn.remap_to)  # overwrites the id
            self.each("move_state", 7, scn.remap_to)
            self.each("set_template", scn.remap_to, scn.conns[7]["reply_tmpl"])
            self.each("set_template", 7, scn.poison_tmpl)
            self.cid[7] = scn.remap_to
            steps.append("remap")
        if steps:
            self.each("table_commit")
        return steps

    # ---- the sender
    def begin_ring(self):
        scn, rng, r = self.scn, self.rng, self.r
        lists, spare, damage, rewrite = [], 0, [], {}
        for c, cn in enumerate(scn.conns):
            if c in self.aborted:
                continue
            entries = []
            for i in range(self.una[c], min(self.una[c] + W, cn["n_img"])):
                off, ln = cn["base"] + i * cn["stride"], int(cn["lens"][i])
                x = rng.random()
                if x < P_DROP:
                    self.cov["dropped"][c] += 1
                    continue
                if off not in rewrite:
                    bad = rng.random() < P_BAD_ACK
                    rewrite[off] = (ln, cn["snd_nxt"] + 1 if bad else scn.ack_at(c, r))
                    self.rewrites[off] = self.rewrites.get(off, 0) + 1
                e = (c, i, off, ln, rewrite[off][1])
                if x < P_DROP + P_DUP:
                    self.cov["duplicated"][c] += 1
                    entries += [e, e]
                elif x < P_DROP + P_DUP + P_DAMAGE and spare < SPARE_SLOTS:
                    at = scn.spare_base + spare * SPARE_STRIDE
                    spare += 1
                    damage.append((off, at, ln, int(rng.integers(0, ln)), int(rng.integers(0, 8))))
                    self.cov["damaged"][c] += 1
                    entries.append((c, i, at, ln, rewrite[off][1]))
                else:
                    entries.append(e)
            for j in range(len(entries) - 1):
                if rng.random() < P_SWAP and entries[j][1] != entries[j + 1][1]:
                    entries[j], entries[j + 1] = entries[j + 1], entries[j]
                    self.cov["swapped"][c] += 1
            if entries:
                lists.append(entries)
        # the peers without a table entry; in two rings a SYN to the listener among them
        ex = [j for j in rng.permutation(12)[:int(rng.integers(4, 8))]]
        if r in SYN_RINGS:
            good = [j for j in range(12) if not scn.extras[j]["bad"]]
            ex = [good[0], ex[0], good[1], 12, good[2], ex[1], good[3]]
        lists.append([(-1, j, scn.extras[j]["off"], scn.extras[j]["len"], scn.extras[j]["ack"]) for j in ex])
        which, idx = interleave(rng, [len(x) for x in lists])
        ring = [lists[w][i] for w, i in zip(which, idx)]
        R = Ring()
        R.n = len(ring)
        assert R.n <= MAX_RING
        R.owner = np.asarray([e[0] for e in ring], np.int64)
        R.idx = np.asarray([e[1] for e in ring], np.int64)
        R.offsets = np.asarray([e[2] for e in ring], np.uint64)
        R.lengths = np.asarray([e[3] for e in ring], np.uint32)
        R.ack = np.asarray([e[4] for e in ring], np.int64)
        R.rw_off = np.asarray(sorted(rewrite), np.uint64)
        R.rw_len = np.asarray([rewrite[o][0] for o in sorted(rewrite)], np.uint32)
        R.rw_ack = np.asarray([rewrite[o][1] for o in sorted(rewrite)], np.uint32)
        R.damage = damage
        self.sizes.append(R.n)
        return R

    # ---- the sender closing the loop, then the application
    def end_ring(self, R, out):
        scn, n, cov = self.scn, R.n, self.cov
        ok, verdict = out["ok"][:n], out["verdict"]
        # every image that arrived whole carries the acknowledgement number the sender wrote this ring
        _, _, h_ack, _, _ = header_fields(out["hdr"][:32 * n])
        good = ok == 1
        assert np.array_equal(h_ack[good], R.ack[good]), "an image was not rewritten"
        known = np.asarray([o >= 0 and o in self.in_table for o in R.owner])
        # an ack number above snd_nxt is never accepted, even in sequence
        for c in set(R.owner[R.owner >= 0].tolist()):
            nxt, cn = self.una[c], scn.conns[c]
            for k in np.flatnonzero(R.owner == c):
                if R.ack[k] > cn["snd_nxt"]:
                    assert not verdict[k] & ACCEPT
                    if ok[k] and R.idx[k] == nxt and known[k] and nxt < cn["n_data"] and not self.stopped(c):
                        cov["bad_ack_rejected"] += 1
                elif verdict[k] & ACCEPT:
                    nxt += 1
        for k in range(n):
            if R.owner[k] < 0 and verdict[k] == HOST:
                cov["listener_host" if scn.extras[R.idx[k]]["syn"] else "unknown_host"] += 1
        # the replies, from their bytes
        total = int(out["count"][0])
        assert 0 <= total <= n
        rows = out["replies"][:32 * total].reshape(-1, 32)
        rst_seen = set()
        for j in range(total):
            row, k = rows[j], int(out["src"][j])
            assert k < n
            if row[25] == 0x20:  # RST: zero addresses and ports, seq = the datagram's acknowledgement number
                assert not row[0:8].any() and not row[12:16].any()
                assert not known[k] and ok[k], "an RST for a datagram of a connection in the table"
                assert _be32(row, 16) == R.ack[k]
                if R.owner[k] < 0:
                    cov["unknown_rst"] += 1
                else:
                    rst_seen.add(int(R.owner[k]))
                continue
            c = self.by_ports.get((int(row[12]) << 8 | int(row[13]), int(row[14]) << 8 | int(row[15])))
            assert c is not None and c in self.in_table, "an ACK from no connection of the table"
            assert R.owner[k] == c and row[25] & F_ACK
            cn = scn.conns[c]
            delta = (_be32(row, 20) - cn["iss"]) & M32  # serial-number arithmetic from the initial sequence number
            assert delta <= cn["data_bytes"] and (delta == cn["P"] or delta % cn["seg"] == 0)
            self.una[c] = max(self.una[c], cn["n_img"] if delta == cn["P"] else delta // cn["seg"])
        for c in rst_seen:
            cov["rst_before_set" if scn.conns[c]["role"] == "late" else "rst_after_erase"] += 1
            self.rst_rings[c] += 1
            if scn.conns[c]["role"] == "erased" and self.rst_rings[c] >= RST_RINGS_BEFORE_ABORT:
                self.aborted.add(c)
        # the application
        st = self.backends[0].get_state(self.cid[3])
        if self.drained_last and st["delivered"] > 0:
            cov["resumed"] += 1
        self.drained_last = st["stopped_at"] != NOT_STOPPED
        if self.drained_last:
            cov["full_drains"] += 1
            self.each("drain", 3, self.cid[3])
        if self.backends[0].get_state(self.cid[4])["stopped_at"] != NOT_STOPPED:
            cov["fin_stops"] += 1
            if not self.fin_host:
                self.each("set_flags", self.cid[4], CONN_HOST)
                self.fin_host = True
        elif self.fin_host:
            cov["fin_host"] += int(((R.owner == 4) & (verdict == HOST)).sum())
        self.r += 1

    def stopped(self, c):
        return self.backends[0].get_state(self.cid[c])["stopped_at"] != NOT_STOPPED

    def done(self):
        return all(self.una[c] >= cn["n_data"] for c, cn in enumerate(self.scn.conns) if cn["role"] != "erased")

    # ---- the end
    def final_checks(self, b):
        scn, recv = self.scn, b.recv_host()
        untouched = np.ones(recv.size, bool)
        for c, cn in enumerate(scn.conns):
            lo, hi = cn["recv_base"], cn["recv_base"] + cn["recv_bytes"]
            st = b.get_state(self.cid[c])
            if cn["role"] == "erased":
                _, window, state = self.erased
                assert np.array_equal(recv[lo:hi], window), "the erased connection's window changed"
                assert st == state, "the erased connection's state changed"
                assert st["delivered"] > 0 and np.array_equal(recv[lo:lo + st["delivered"]], cn["stream"][:st["delivered"]])
                untouched[lo:lo + st["delivered"]] = False
                continue
            got = bytes(b.log[c]) + recv[lo:lo + st["delivered"]].tobytes()
            assert got == cn["stream"][:cn["data_bytes"]].tobytes(), f"connection {c}: the receive stream is not the send stream"
            assert st["rcv_nxt"] == (cn["iss"] + cn["data_bytes"]) & M32
            untouched[lo:hi if cn["role"] == "small_window" else lo + st["delivered"]] = False
        assert (recv[untouched] == SENTINEL).all(), "a sentinel byte of the shared receive buffer changed"


def run(scn, backends, per_ring=None, want_rings=None):
    """The loop to its end on backends that advance together; per_ring(loop, R, outs) after every
    ring (before the sender reads the replies).  Returns the Loop."""
    loop = Loop(scn, backends)
    loop.start()
    while not loop.done():
        assert loop.r < HARD_STOP, "the loop does not end"
        steps = loop.control()
        R = loop.begin_ring()
        outs = [b.ring(R) for b in backends if not isinstance(b, LibTwin)]
        if per_ring:
            per_ring(loop, R, outs, steps)
        loop.end_ring(R, outs[0])
    for b in backends:
        if not isinstance(b, LibTwin):
            loop.final_checks(b)
    if want_rings is not None:
        assert loop.r == want_rings, (loop.r, want_rings)
    return loop
