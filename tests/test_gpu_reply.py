"""GPU tests of the batched reply builder: tcpck_batch_reply compared bit-exactly
with its host twin tcpck_build_replies and with the numpy restatement
(tests/reply_np.py), on the reference's own datagrams (tests/golden/reply_golden.*),
over the counts at which the launch changes shape, reply patterns that leave
waves and blocks empty, the bounds of everything it writes, and the whole ring
path receive -> demux -> plan -> deliver + reply on the golden ring."""
import ctypes

import numpy as np
import pytest

from deliver_np import SKIP, DeliverGolden
from demux_np import PORT_1, STATE_KEYS, check_golden_ring, golden_ring, header_keys, set_port
from reply_np import HOST, NONE, RST, SEND_ACK, ReplyGolden, random_ring, reply_np, template_np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = (0, 1)
GUARD = 64           # guard elements after every output array
FILL = 0xA5
BLOCK = 1024         # images per block of the count and emit passes (tcpck_reply.h)
SCAN = 1024          # block totals the scan takes per step: above BLOCK * SCAN images it carries
# 1 .. 4099: one wave, one block, the block edges; 2^20 + 3: 1025 blocks, the scan's second step
COUNTS = (1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 4099)
BIG = (1 << 20) + 3


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available()
    c = tcpck.Context(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def as_i32(a):
    return np.ascontiguousarray(a, np.uint32).view(np.int32)


class Call:
    """One tcpck_batch_reply: the inputs uploaded (the templates in an allocation of exactly 32 *
    n_conns bytes), every output with GUARD sentinel elements after it.  check() reads everything
    back and compares whole arrays."""

    def __init__(self, ctx, verdict, ack, conn, tmpl, n_conns, cap, mode, stream=None, with_src=True):
        import tcpck
        self.args = (verdict, ack, conn, tmpl, n_conns, cap, mode)
        n = len(verdict)
        self.d_verdict, self.d_ack = dev(verdict), dev(as_i32(ack))
        self.d_conn = None if conn is None else dev(as_i32(conn))
        self.d_tmpl = dev(np.asarray(tmpl, np.uint8)[:32 * n_conns]) if n_conns else None
        self.d_replies = torch.full((32 * (cap + GUARD),), FILL, dtype=torch.uint8, device="cuda")
        self.d_src = torch.full((cap + GUARD,), -1, dtype=torch.int32, device="cuda") if with_src else None
        self.d_count = torch.full((1 + GUARD,), -1, dtype=torch.int64, device="cuda")
        self.scratch_bytes = tcpck.reply_scratch_bytes(n)
        self.d_scratch = torch.full((self.scratch_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.batch_reply(self.d_verdict, self.d_ack, self.d_tmpl, n_conns, n, self.d_replies, cap, self.d_count,
                        self.d_scratch, conn=self.d_conn, src=self.d_src, mode=mode, stream=stream)

    def check(self, twin=True):
        import tcpck
        verdict, ack, conn, tmpl, n_conns, cap, mode = self.args
        torch.cuda.synchronize()
        exp, exp_src, total = reply_np(verdict, ack, conn, tmpl, n_conns, cap, mode)
        if twin:
            got = tcpck.build_replies(verdict, ack, np.asarray(tmpl, np.uint8)[:32 * n_conns], conn=conn, reply_cap=cap,
                                      mode=mode)
            assert got[2] == total and np.array_equal(got[0], exp) and np.array_equal(got[1], exp_src)
        w = min(total, cap)
        count = self.d_count.cpu().numpy()
        assert count[0] == total and (count[1:] == -1).all(), "d_count or the bytes after it"
        replies = self.d_replies.cpu().numpy()
        rows = replies[:32 * w].reshape(-1, 32)
        assert np.array_equal(rows, exp), np.flatnonzero((rows != exp).any(axis=1))[:8]
        assert (replies[32 * w:] == FILL).all(), "written past the last reply"
        if self.d_src is not None:
            src = self.d_src.cpu().numpy()
            assert np.array_equal(src[:w].view(np.uint32), exp_src) and (src[w:] == -1).all(), "d_src or past it"
        assert (self.d_scratch.cpu().numpy()[self.scratch_bytes:] == FILL).all(), "written past the scratch"
        # the inputs are only read
        assert np.array_equal(self.d_verdict.cpu().numpy(), verdict)
        assert np.array_equal(self.d_ack.cpu().numpy().view(np.uint32), ack)
        if conn is not None:
            assert np.array_equal(self.d_conn.cpu().numpy().view(np.uint32), conn)
        if n_conns:
            assert np.array_equal(self.d_tmpl.cpu().numpy(), np.asarray(tmpl, np.uint8)[:32 * n_conns])
        return rows, total


def pattern(name, count, seed=0):
    """Which images reply."""
    k = np.arange(count)
    rng = np.random.default_rng(seed)
    if name == "none":
        return np.zeros(count, bool)
    if name == "all":
        return np.ones(count, bool)
    if name == "first":
        return k == 0
    if name == "last":
        return k == count - 1
    if name == "alternating":
        return k % 2 == 1
    if name in ("per64", "per256"):
        step = int(name[3:])
        return k % step == (step // 3)
    if name in ("gaps64", "gaps256"):  # silent runs of exactly one wave / one wave's four chunks: start, middle, end
        run = int(name[4:])
        m = np.ones(count, bool)
        for at in (0, (count // 2) // run * run, max(0, (count - run) // run * run), max(0, count - run)):
            m[at:at + run] = False
        return m
    return rng.random(count) < {"p10": 0.1, "p50": 0.5, "p90": 0.9}[name]


PATTERNS = ("none", "all", "first", "last", "alternating", "per64", "per256", "gaps64", "gaps256", "p10", "p50", "p90")


def ring_for(mask, kinds, seed, n_conns, bad_ids=False):
    """verdict / ack / conn / tmpl for a reply mask.  kinds: 'rst', 'ack' or 'mixed' (ACKs of every
    verdict value the planners give, RSTs, and HOST / zero / accept-only verdicts where silent)."""
    count = mask.size
    _, ack, conn, tmpl = random_ring(seed, count, n_conns, bad_ids=False)
    rng = np.random.default_rng(seed + 1)
    silent = np.asarray([0, 1, 3, HOST, 8, HOST | 1], np.uint8)[rng.integers(0, 6, count)]
    acks = np.asarray([7, 5, 12, 4], np.uint8)[rng.integers(0, 4, count)]
    if kinds == "rst":
        loud = np.full(count, RST, np.uint8)
    elif kinds == "ack":
        loud = acks
    else:
        loud = np.where(rng.random(count) < 0.25, np.uint8(RST), acks).astype(np.uint8)
        loud[rng.random(count) < 0.05] = RST | SEND_ACK
    verdict = np.where(mask, loud, silent).astype(np.uint8)
    if bad_ids:  # ids that name no template, under SEND_ACK too: those images fall silent
        bad = rng.random(count) < 0.25
        conn[bad] = np.asarray([NONE, n_conns, n_conns + 1, 0x80000000, NONE - 1], np.uint32)[
            rng.integers(0, 5, int(bad.sum()))]
    return verdict, ack, conn, tmpl


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", COUNTS)
def test_counts(ctx, count, mode):
    for i, name in enumerate(("all", "p50", "last", "none")):
        verdict, ack, conn, tmpl = ring_for(pattern(name, count, count), "mixed", 10 * count + i, 7)
        rows, total = Call(ctx, verdict, ack, conn, tmpl, 7, count, mode).check()
        if name == "all":
            assert total == count
        if name == "none":
            assert total == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", PATTERNS)
def test_patterns(ctx, name, mode):
    """4099 images (five blocks, the last nearly empty) and 2600: empty waves and empty blocks at
    the start, the middle and the end."""
    for count in (4099, 2600):
        mask = pattern(name, count, 5)
        for kinds in ("mixed", "rst", "ack"):
            verdict, ack, conn, tmpl = ring_for(mask, kinds, count + len(name), 7)
            rows, total = Call(ctx, verdict, ack, conn, tmpl, 7, count, mode).check()
            assert total == int(mask.sum())
            if total and kinds != "mixed":
                assert (rows[:, 25] == 0x20).all() == (kinds == "rst")


@pytest.mark.parametrize("mode", MODES)
def test_scan_second_step(ctx, mode):
    """2^20 + 3 images: 1025 blocks, so the scan of the block totals takes a second step with a
    carry, and the last block holds three images."""
    verdict, ack, conn, tmpl = ring_for(pattern("p50", BIG, 77), "mixed", 77, 4096)
    assert BIG > BLOCK * SCAN
    c = Call(ctx, verdict, ack, conn, tmpl, 4096, BIG, mode)
    rows, total = c.check()
    assert verdict[-3:].tolist() and total > BIG // 3
    assert c.scratch_bytes == 4 * 1028  # 1025 block totals, rounded up to 16 B


@pytest.mark.parametrize("mode", MODES)
def test_connections(ctx, mode):
    count = 3000
    mask = pattern("p90", count, 3)
    # no ids: every image is connection 0
    verdict, ack, _, tmpl = ring_for(mask, "mixed", 1, 1)
    Call(ctx, verdict, ack, None, tmpl, 1, count, mode).check()
    # ... which a call without templates does not have: only the RSTs reply
    rows, total = Call(ctx, verdict, ack, None, tmpl, 0, count, mode).check()
    assert total == int(((verdict & RST) != 0).sum()) > 0 and (rows[:, 25] == 0x20).all()
    for n_conns in (1, 7, 4096):
        verdict, ack, conn, tmpl = ring_for(mask, "mixed", 2 + n_conns, n_conns)
        Call(ctx, verdict, ack, conn, tmpl, n_conns, count, mode).check()
        # ids NONE and >= n_conns under SEND_ACK: silent, the templates' allocation is exactly theirs
        verdict, ack, conn, tmpl = ring_for(mask, "ack", 3 + n_conns, n_conns, bad_ids=True)
        rows, total = Call(ctx, verdict, ack, conn, tmpl, n_conns, count, mode).check()
        assert total == int((mask & (conn < n_conns)).sum()) < int(mask.sum())


@pytest.mark.parametrize("mode", MODES)
def test_fixture_ring(ctx, mode):
    """The reference's own ACK and RST datagrams (REF), and tcpck_fill16's RFC 1071 checksums on them."""
    import tcpck
    rg = ReplyGolden()
    verdict, ack, conn, tmpl = rg.ring()
    n = len(rg.cases)
    rows, total = Call(ctx, verdict, ack, conn, tmpl, n, n, mode).check()
    assert total == n and np.array_equal(rows, rg.images if mode == 0 else rg.rfc_images(tcpck.fill16))


@pytest.mark.parametrize("mode", MODES)
def test_reply_cap(ctx, mode):
    count = 2500
    verdict, ack, conn, tmpl = ring_for(pattern("p50", count, 8), "mixed", 8, 7)
    total = reply_np(verdict, ack, conn, tmpl, 7, count, mode)[2]
    for cap in (0, 1, total - 1, total, total + 1):
        assert Call(ctx, verdict, ack, conn, tmpl, 7, cap, mode).check()[1] == total
    Call(ctx, verdict, ack, conn, tmpl, 7, total - 1, mode, with_src=False).check()


def test_count_zero(ctx):
    import tcpck
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ctx._L.tcpck_batch_reply(ctx._h, 0, None, None, None, None, 0, 0, None, 0, None, d_count.data_ptr(), None,
                                    None) == tcpck.OK
    torch.cuda.synchronize()
    assert d_count.cpu().tolist() == [0, -1]
    assert ctx._L.tcpck_batch_reply(ctx._h, 0, None, None, None, None, 0, 0, None, 0, None, None, None, None) == tcpck.OK


def test_two_streams(ctx):
    """Two calls on two streams into different outputs, nothing waited for in between."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = ring_for(pattern("p50", 70000, 1), "mixed", 1, 7)
    b = ring_for(pattern("p90", 50001, 2), "mixed", 2, 40)
    c1 = Call(ctx, *a, 7, 70000, 0, stream=s1)
    c2 = Call(ctx, *b, 40, 50001, 1, stream=s2)
    c1.check()
    c2.check()
    # and the same inputs give the same bytes again
    c3 = Call(ctx, *a, 7, 70000, 0, stream=s2)
    c3.check(twin=False)
    assert torch.equal(c1.d_replies, c3.d_replies) and torch.equal(c1.d_src, c3.d_src)


@pytest.mark.parametrize("mode", MODES)
def test_replies_verify(ctx, mode):
    """Round trip: the reply ring through tcpck_batch_fixed(VERIFY, stride 32, len 32) in the mode
    it was built in."""
    import tcpck
    count = 5000
    verdict, ack, conn, tmpl = ring_for(pattern("p90", count, 4), "mixed", 4, 7)
    c = Call(ctx, verdict, ack, conn, tmpl, 7, count, mode)
    rows, total = c.check()
    ok = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ctx.batch_fixed(tcpck.OP_VERIFY, c.d_replies, 32, 32, total, ok, mode=mode)
    torch.cuda.synchronize()
    assert bool(ok.all().item())


def test_golden_ring_end_to_end(ctx):
    """The reference's two arrival sequences interleaved in one ring with datagrams of no socket
    among them, every device call on ONE stream: receive -> demux, the copy down that the host
    planner needs, plan_deliver_multi, the 13 B per image back up, then deliver AND reply with
    nothing waited for until the final read-back.  The receive windows are the reference's
    recv_buffers, and the reply ring holds one ACK per SendAck the reference made, with its numbers,
    and one RST per good datagram of no socket."""
    import tcpck
    dg = DeliverGolden()
    ring = golden_ring(dg, tcpck.update16)
    s0, s1 = dg.sequences
    wire, offsets, lengths, which = ring["wire"], ring["offsets"].tolist(), ring["lengths"].tolist(), ring["which"].tolist()
    donors = [i for i in range(len(s0["offsets"])) if s0["ok"][i] and s0["lengths"][i] > 100][:4]
    good = []
    for j, (i, at) in enumerate(zip(donors, (0, 20, 51, len(which) + 3))):
        img = dg.wire(s0)[s0["offsets"][i]:s0["offsets"][i] + s0["lengths"][i]].copy()
        set_port(img, 0, 14, 15999, tcpck.update16)  # a port nobody listens on
        if j == 1:
            img[50] ^= 0x10
        good.append(j != 1)
        offsets.insert(at, wire.size)
        lengths.insert(at, img.size)
        which.insert(at, 2)
        wire = np.concatenate([wire, img])
    ring = dict(wire=wire, offsets=np.asarray(offsets, np.uint64), lengths=np.asarray(lengths, np.uint32),
                which=np.asarray(which))
    n = len(which)
    bases = (0, (s0["recv_bytes"] + 65) & ~1)
    recv_total = bases[1] + s1["recv_bytes"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_wire, d_off, d_len = dev(wire), dev(ring["offsets"]), dev(ring["lengths"])
        d_ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_hdr = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        d_conn = torch.full((n,), -2, dtype=torch.int32, device="cuda")
        d_recv = torch.full((recv_total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        d_replies = torch.full((32 * (n + GUARD),), FILL, dtype=torch.uint8, device="cuda")
        d_src = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        d_scratch = torch.empty(tcpck.reply_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        with tcpck.ConnTable(ctx, 8) as t:
            ctx.batch_receive(d_wire, n, d_ok, d_hdr, offsets=d_off, lengths=d_len, stream=stream)
            hdr = d_hdr.cpu().numpy()  # (receive is done: the keys for the table come from its headers)
            host_port, peer_ip, peer_port, _ = header_keys(hdr)
            key = lambda c: next((int(host_port[k]), int(peer_ip[k]), int(peer_port[k])) for k in range(n) if which[k] == c)
            assert key(1)[2] == PORT_1
            t.set(*key(0), 0)
            t.set(*key(1), 1)
            t.commit(stream)
            ctx.batch_demux(t, d_hdr, n, d_conn, stream=stream)
            ok, conn = d_ok.cpu().numpy(), d_conn.cpu().numpy().view(np.uint32)  # the copy down for the planner
        conns = (tcpck.ConnState * 2)(*[
            tcpck.ConnState(tcpck.RcvState(*(s["initial"][k] for k in STATE_KEYS[:4]), 0, 0), b, s["recv_bytes"], 0, 0, 0)
            for s, b in zip(dg.sequences, bases)])
        dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=ring["lengths"])
        tmpl = np.concatenate([template_np(s["initial"]["snd_nxt"], s["initial"]["snd_wnd"], 0x7F000001, 15501, 0x7F000001,
                                           port) for s, port in zip(dg.sequences, (15500, PORT_1))])
        d_dst, d_verdict, d_ack, d_tmpl = dev(dst.view(np.int64)), dev(verdict), dev(as_i32(ack)), dev(tmpl)
        ctx.batch_deliver(d_wire, n, d_dst, d_recv, recv_total, offsets=d_off, lengths=d_len, stream=stream)
        ctx.batch_reply(d_verdict, d_ack, d_tmpl, 2, n, d_replies, n, d_count, d_scratch, conn=d_conn, src=d_src,
                        stream=stream)
        stream.synchronize()  # the only wait after the plan
    check_golden_ring(dg, ring, hdr, ok, conn, dst, verdict, ack, conns)
    got = d_recv.cpu().numpy()
    assert np.array_equal(got[:s0["recv_bytes"]], dg.recv(s0)) and np.array_equal(got[bases[1]:recv_total], dg.recv(s1))
    assert (got[s0["recv_bytes"]:bases[1]] == FILL).all() and (got[recv_total:] == FILL).all()
    exp, exp_src, total = reply_np(verdict, ack, conn, tmpl, 2, n, 0)
    assert d_count.cpu().tolist() == [total, -1]
    replies = d_replies.cpu().numpy()
    assert np.array_equal(replies[:32 * total].reshape(-1, 32), exp) and (replies[32 * total:] == FILL).all()
    src = d_src.cpu().numpy()
    assert np.array_equal(src[:total].view(np.uint32), exp_src) and (src[total:] == -1).all()
    # against the reference's records: per connection one ACK per SendAck before its walk stopped
    be = lambda rows: (rows.astype(np.uint32) << np.asarray([24, 16, 8, 0], np.uint32)).sum(axis=1)
    n_acks = 0
    for c, s in enumerate(dg.sequences):
        at_ring = np.flatnonzero(ring["which"] == c)
        stop = s["left_estab_at"] if s["left_estab_at"] >= 0 else len(at_ring)
        sent = [i for i in range(stop) if s["send_ack"][i]]
        mine = np.flatnonzero(np.isin(exp_src, at_ring))
        assert exp_src[mine].tolist() == at_ring[sent].tolist()
        assert be(exp[mine, 16:20]).tolist() == [s["reply_seq"][i] for i in sent]
        assert be(exp[mine, 20:24]).tolist() == [s["reply_ack"][i] for i in sent]
        assert (exp[mine, 25] == 0x08).all()
        n_acks += len(sent)
    unknown = np.flatnonzero(ring["which"] == 2)
    rst = np.flatnonzero(exp[:, 25] == 0x20)
    assert exp_src[rst].tolist() == unknown[good].tolist() and total == n_acks + 3
    assert all(tcpck.checksum16(r) == 0 for r in exp)
    assert (dst[unknown] == SKIP).all() and np.array_equal(d_wire.cpu().numpy(), wire)


def test_argument_checks(ctx):
    """Every TCPCK_EINVAL clause: nothing is launched, so no output changes."""
    import tcpck
    L = ctx._L
    n = 300
    verdict, ack, conn, tmpl = ring_for(pattern("all", n), "mixed", 6, 4)
    d_verdict, d_ack, d_conn, d_tmpl = dev(verdict), dev(as_i32(ack)), dev(as_i32(conn)), dev(np.tile(tmpl, 2))
    d_replies = torch.full((32 * (n + 1),), FILL, dtype=torch.uint8, device="cuda")
    d_src = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda")
    d_count = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((tcpck.reply_scratch_bytes(n) + 32,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    good = dict(ctx=ctx._h, mode=0, verdict=d_verdict.data_ptr(), ack=d_ack.data_ptr(), conn=d_conn.data_ptr(),
                tmpl=d_tmpl.data_ptr(), n_conns=4, count=n, replies=d_replies.data_ptr(), cap=n, src=d_src.data_ptr(),
                total=d_count.data_ptr(), scratch=d_scratch.data_ptr(), stream=None)
    call = lambda **kw: L.tcpck_batch_reply(*{**good, **kw}.values())
    bad = [dict(ctx=None), dict(mode=2), dict(mode=-1), dict(count=(1 << 31) + 1), dict(verdict=None), dict(ack=None),
           dict(replies=None), dict(total=None), dict(scratch=None), dict(tmpl=None), dict(ack=good["ack"] + 2),
           dict(conn=good["conn"] + 1), dict(src=good["src"] + 2), dict(tmpl=good["tmpl"] + 8),
           dict(replies=good["replies"] + 8), dict(scratch=good["scratch"] + 4), dict(total=good["total"] + 4),
           dict(count=0, mode=9), dict(count=0, total=good["total"] + 2)]
    for kw in bad:
        assert call(**kw) == tcpck.EINVAL, kw
    torch.cuda.synchronize()
    assert (d_replies.cpu().numpy() == FILL).all() and (d_src.cpu().numpy() == -1).all()
    assert d_count.cpu().tolist() == [-1, -1, -1] and (d_scratch.cpu().numpy() == FILL).all()
    # the alignments that are enough: 4 B for the u32 arrays, 16 B for templates, replies and scratch, 8 B for the count
    assert call(ack=good["ack"] + 4, conn=good["conn"] + 4, src=good["src"] + 4, tmpl=good["tmpl"] + 16,
                replies=good["replies"] + 16, scratch=good["scratch"] + 16, total=good["total"] + 8, count=n - 1,
                cap=n - 1) == tcpck.OK
    torch.cuda.synchronize()
    exp, exp_src, total = reply_np(verdict[:n - 1], ack[1:], conn[1:], np.tile(tmpl, 2)[16:], 4, n - 1, 0)
    assert d_count.cpu().tolist() == [-1, total, -1]
    got = d_replies.cpu().numpy()
    assert (got[:16] == FILL).all() and np.array_equal(got[16:16 + 32 * total].reshape(-1, 32), exp)
    assert (got[16 + 32 * total:] == FILL).all()
    src = d_src.cpu().numpy()
    assert src[0] == -1 and np.array_equal(src[1:1 + total].view(np.uint32), exp_src) and (src[1 + total:] == -1).all()
    # reply_scratch_bytes is a function of the count alone, and what the launcher uses
    out = ctypes.c_size_t()
    assert L.tcpck_reply_scratch_bytes(n, ctypes.byref(out)) == tcpck.OK and out.value == 16
