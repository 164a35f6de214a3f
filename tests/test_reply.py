"""CPU tests of the batched reply builder's host side: tcpck_build_replies and the
numpy restatement tests/reply_np.py against the datagrams the reference's own
helpers build (tests/golden/reply_golden.*, from tests/golden/gen_reply.cc),
against each other on seeded rings, behind both receive planners, and every
argument rule.  No GPU call here."""
import ctypes

import numpy as np
import pytest

from deliver_np import DeliverGolden
from demux_np import CONN_HOST, mixed_ring
from reply_np import HOST, NONE, RST, SEND_ACK, ReplyGolden, random_ring, reply_np, template_np

MODES = (0, 1)


@pytest.fixture(scope="module")
def rg():
    return ReplyGolden()


def both(tcpck, verdict, ack, conn, tmpl, n_conns, cap, mode):
    """tcpck_build_replies and reply_np on the same ring, compared; -> (replies, src, total)."""
    got = tcpck.build_replies(verdict, ack, tmpl[:32 * n_conns], conn=conn, reply_cap=cap, mode=mode)
    exp = reply_np(verdict, ack, conn, tmpl, n_conns, cap, mode)
    assert got[2] == exp[2]
    assert np.array_equal(got[0], exp[0]), np.flatnonzero((got[0] != exp[0]).any(axis=1))[:8]
    assert np.array_equal(got[1], exp[1])
    return got


def test_fixture_examples(rg):
    """The two datagrams the reference's helpers printed for the issue, found in the fixture."""
    by = {(c["kind"], c["group"]): rg.images[k] for k, c in enumerate(rg.cases)}
    want = "00000001 00000000 00000000 00020000 00000005 00000007 00080009 ffdf0000".replace(" ", "")
    assert by[("ack", "example")].tobytes().hex() == want
    r = by[("rst", "example")]
    assert r[16:20].tolist() == [1, 2, 3, 4] and r[25] == 0x20
    assert not r[:16].any() and not r[20:25].any() and not r[26:28].any() and not r[30:].any()


def test_fixture_covers_what_it_should(rg):
    groups = {c["group"] for c in rg.cases}
    assert {"checksum-0000", "checksum-ffff", "carries", "random", "edge-seq", "edge-all"} <= groups
    kinds = [c["kind"] for c in rg.cases]
    assert 200 <= len(kinds) <= 300 and kinds.count("rst") >= 40
    # interleaved: no long run of one kind
    runs = np.diff(np.flatnonzero(np.diff(np.asarray([k == "rst" for k in kinds], int)) != 0))
    assert runs.max() < 40
    stored = np.asarray([c["ref_checksum"] for c in rg.cases])
    assert (stored == 0).sum() >= 20 and (stored == 0xFFFF).sum() >= 20
    assert sum(c["word_sum"] >> 16 >= 2 for c in rg.cases) >= 30
    edge = {0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x00FF00FF, 0xFF00FF00}
    for key in ("seq", "ack", "src_ip", "dst_ip"):
        assert edge <= {c[key] for c in rg.cases}, key


@pytest.mark.parametrize("mode", MODES)
def test_fixture_ring(built_lib, rg, mode):
    """The whole fixture as one mixed ring, connection k = case k's template."""
    import tcpck
    verdict, ack, conn, tmpl = rg.ring()
    n = len(rg.cases)
    replies, src, total = both(tcpck, verdict, ack, conn, tmpl, n, n, mode)
    assert total == n and np.array_equal(src, np.arange(n))
    want = rg.images if mode == 0 else rg.rfc_images(tcpck.fill16)
    assert np.array_equal(replies, want), np.flatnonzero((replies != want).any(axis=1))[:8]
    if mode == 1:  # the carrying cases: the two modes store different checksums
        differ = (want[:, 28:30] != rg.images[:, 28:30]).any(axis=1)
        assert differ[[c["word_sum"] >> 16 >= 2 for c in rg.cases]].all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count,n_conns,seed", [(1, 1, 1), (64, 1, 2), (1000, 7, 3), (5000, 4096, 4), (3000, 40, 5)])
def test_seeded_rings(built_lib, count, n_conns, seed, mode):
    import tcpck
    verdict, ack, conn, tmpl = random_ring(seed, count, n_conns, bad_ids=seed == 5)
    replies, src, total = both(tcpck, verdict, ack, conn, tmpl, n_conns, count, mode)
    assert total == src.size
    if count >= 1000:
        assert 0 < total < count and (replies[:, 25] == 0x20).any() and (replies[:, 25] != 0x20).any()
    # every reply verifies in the mode it was built in
    assert all(tcpck.checksum16(r, mode) == 0 for r in replies[:200])
    # no connection ids: every image is connection 0
    both(tcpck, verdict, ack, None, tmpl, n_conns, count, mode)


def test_rst_wins_over_send_ack_and_silent_verdicts(built_lib):
    import tcpck
    verdict = np.asarray([RST | SEND_ACK, SEND_ACK, 0, HOST, 1, 3, 8, RST, HOST | 1], np.uint8)
    ack = np.arange(9, dtype=np.uint32) + 0x01020300
    conn = np.asarray([NONE, 0, 0, 0, 0, 0, 0, 5, 0], np.uint32)
    tmpl = template_np(77, 9, 1, 2, 3, 4)
    replies, src, total = both(tcpck, verdict, ack, conn, tmpl, 1, 9, 0)
    assert src.tolist() == [0, 1, 7] and total == 3
    assert replies[0, 25] == 0x20 and replies[1, 25] == 0x08 and replies[2, 25] == 0x20
    assert not replies[0, :16].any() and replies[0, 16:20].tolist() == [1, 2, 3, 0]
    assert replies[1, 20:24].tolist() == [1, 2, 3, 1] and np.array_equal(replies[1, :20], tmpl[:20])


@pytest.mark.parametrize("mode", MODES)
def test_behind_the_single_planner(built_lib, mode):
    """tcpck_plan_deliver on both golden sequences, then the replies from its verdict / ack with a
    template carrying the sequence's snd_nxt / snd_wnd: one reply per SendAck the reference made,
    with the seq and ack numbers it passed."""
    import tcpck
    dg = DeliverGolden()
    for s in dg.sequences:
        hdr, ok = dg.host_headers(dg.wire(s), s["offsets"], s["lengths"])
        init = s["initial"]
        st = tcpck.RcvState(init["rcv_nxt"], init["snd_nxt"], init["snd_una"], init["rcv_wnd"], 0, 0)
        _, verdict, ack, used = tcpck.plan_deliver(hdr, ok, st, s["recv_bytes"], lengths=np.asarray(s["lengths"], np.uint32))
        tmpl = template_np(init["snd_nxt"], init["snd_wnd"], 0x7F000001, 15501, 0x7F000001, 15500)
        replies, src, total = both(tcpck, verdict, ack, None, tmpl, 1, len(ok), mode)
        # the planner stops before the FIN that leaves Estab (sequence 1's last image): that image and
        # the ACK the reference sends for it are the host state machine's, not this ring's
        assert used == (s["left_estab_at"] if s["left_estab_at"] >= 0 else len(ok))
        sent = np.flatnonzero(np.asarray(s["send_ack"][:used]))
        assert int(np.sum(s["send_ack"][used:])) == (1 if used < len(ok) else 0)
        assert total == int(np.sum(s["send_ack"][:used])) > 10 and np.array_equal(src, sent)
        be = lambda rows: (rows.astype(np.uint32) << np.asarray([24, 16, 8, 0], np.uint32)).sum(axis=1)
        assert be(replies[:, 16:20]).tolist() == [s["reply_seq"][k] for k in sent]
        assert be(replies[:, 20:24]).tolist() == [s["reply_ack"][k] for k in sent]
        assert (replies[:, 25] == 0x08).all()
        assert (be(np.pad(replies[:, 26:28], ((0, 0), (2, 0)))) == init["snd_wnd"]).all()


@pytest.mark.parametrize("mode", MODES)
def test_behind_the_ring_planner(built_lib, mode):
    """A mixed ring through tcpck_plan_deliver_multi with RST and HOST images present."""
    import tcpck
    hdr, ok, lengths, conn, conns = mixed_ring(31, 12, 80)
    for c in conns[3::4]:
        c["flags"] = CONN_HOST
    conn = conn.copy()
    conn[np.random.default_rng(31).random(conn.size) < 0.1] = NONE
    arr = (tcpck.ConnState * len(conns))(*[
        tcpck.ConnState(tcpck.RcvState(d["rcv_nxt"], d["snd_nxt"], d["snd_una"], d["rcv_wnd"], 0, 0), d["recv_base"],
                        d["recv_bytes"], 0, d["flags"], 0) for d in conns])
    _, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, arr, lengths=lengths)
    assert (verdict & RST).any() and (verdict & HOST).any() and (verdict & SEND_ACK).any() and (verdict == 0).any()
    tmpl = np.concatenate([template_np(d["snd_nxt"], 4096, 0x0A000001, 80, 0x0A000002 + i, 4000 + i)
                           for i, d in enumerate(conns)])
    replies, src, total = both(tcpck, verdict, ack, conn, tmpl, len(conns), len(ok), mode)
    want = (verdict & (RST | SEND_ACK)) != 0
    assert np.array_equal(src, np.flatnonzero(want)) and total == int(want.sum())
    is_rst = (verdict[src] & RST) != 0
    assert np.array_equal(replies[:, 25] == 0x20, is_rst) and (conn[src[is_rst]] == NONE).all()
    assert (conn[src[~is_rst]] != NONE).all()
    # an ACK carries its own connection's ports
    ports = replies[~is_rst, 14].astype(int) << 8 | replies[~is_rst, 15]
    assert np.array_equal(ports, 4000 + conn[src[~is_rst]])


@pytest.mark.parametrize("mode", MODES)
def test_reply_cap(built_lib, mode):
    """cap = 0, total - 1, total, total + 1: only the first cap replies and src entries are
    written, the total is reported in full, and nothing past them is touched."""
    import tcpck
    L = tcpck.lib()
    verdict, ack, conn, tmpl = random_ring(9, 700, 5)
    full, full_src, total = reply_np(verdict, ack, conn, tmpl, 5, 700, mode)
    assert 100 < total < 600
    for cap in (0, 1, total - 1, total, total + 1, 700):
        replies = np.full((total + 8) * 32, 0xA5, np.uint8)
        src = np.full(total + 8, 0xA5A5A5A5, np.uint32)
        n = ctypes.c_uint64(99)
        assert L.tcpck_build_replies(mode, verdict.ctypes.data, ack.ctypes.data, conn.ctypes.data, tmpl.ctypes.data, 5,
                                     700, replies.ctypes.data, cap, src.ctypes.data, ctypes.byref(n)) == tcpck.OK
        w = min(cap, total)
        assert n.value == total
        assert np.array_equal(replies[:32 * w].reshape(-1, 32), full[:w]) and (replies[32 * w:] == 0xA5).all()
        assert np.array_equal(src[:w], full_src[:w]) and (src[w:] == 0xA5A5A5A5).all()
        both(tcpck, verdict, ack, conn, tmpl, 5, cap, mode)
    # src may be NULL
    replies = np.zeros(total * 32, np.uint8)
    assert L.tcpck_build_replies(mode, verdict.ctypes.data, ack.ctypes.data, conn.ctypes.data, tmpl.ctypes.data, 5, 700,
                                 replies.ctypes.data, total, None, ctypes.byref(n)) == tcpck.OK
    assert np.array_equal(replies.reshape(-1, 32), full)


def test_guard_rails_for_connection_ids(built_lib):
    """SEND_ACK with an id of NONE or >= n_conns: no reply, and no template byte outside
    [0, 32 * n_conns) is read -- the bytes after the templates are poison that would show."""
    import tcpck
    n_conns = 3
    tmpl = np.concatenate([np.random.default_rng(2).integers(0, 256, 32 * n_conns, dtype=np.uint8),
                           np.full(64, 0xEE, np.uint8)])
    conn = np.asarray([0, 1, 2, 3, 4, NONE, 0x80000000, 2, NONE - 1, 0], np.uint32)
    verdict = np.full(conn.size, 5, np.uint8)
    ack = np.arange(conn.size, dtype=np.uint32)
    for mode in MODES:
        replies, src, total = both(tcpck, verdict, ack, conn, tmpl, n_conns, conn.size, mode)
        assert src.tolist() == [0, 1, 2, 7, 9] and total == 5
        assert not (replies[:, :16] == 0xEE).all(axis=1).any()
        # no templates at all: only an RST can reply
        v2 = verdict.copy()
        v2[4] = RST
        L = tcpck.lib()
        out, n = np.zeros(32 * 10, np.uint8), ctypes.c_uint64()
        assert L.tcpck_build_replies(mode, v2.ctypes.data, ack.ctypes.data, conn.ctypes.data, None, 0, conn.size,
                                     out.ctypes.data, 10, None, ctypes.byref(n)) == tcpck.OK
        assert n.value == 1 and out[25] == 0x20 and out[19] == 4
        # and without ids every image is connection 0, which n_conns == 0 does not have
        assert L.tcpck_build_replies(mode, verdict.ctypes.data, ack.ctypes.data, None, None, 0, conn.size,
                                     out.ctypes.data, 10, None, ctypes.byref(n)) == tcpck.OK and n.value == 0


def test_argument_checks_write_nothing(built_lib):
    import tcpck
    L = tcpck.lib()
    verdict, ack, conn, tmpl = random_ring(3, 50, 4)
    raw = np.full(32 * 50 + 64, 0xA5, np.uint8)
    at = (-raw.ctypes.data) % 16
    replies = raw[at:at + 32 * 50 + 16]
    src = np.full(51, 0xA5A5A5A5, np.uint32)
    total = (ctypes.c_uint64 * 2)(77, 77)
    t_raw = np.zeros(32 * 4 + 32, np.uint8)
    t_at = (-t_raw.ctypes.data) % 16
    t = t_raw[t_at:t_at + 32 * 4 + 8]
    t[:32 * 4] = tmpl
    good = dict(mode=0, verdict=verdict.ctypes.data, ack=ack.ctypes.data, conn=conn.ctypes.data, tmpl=t.ctypes.data,
                n_conns=4, count=50, replies=replies.ctypes.data, cap=50, src=src.ctypes.data,
                total=ctypes.addressof(total))
    order = ("mode", "verdict", "ack", "conn", "tmpl", "n_conns", "count", "replies", "cap", "src", "total")

    def call(**kw):
        a = {**good, **kw}
        a["total"] = ctypes.cast(a["total"], ctypes.POINTER(ctypes.c_uint64)) if a["total"] else None
        return L.tcpck_build_replies(*[a[k] for k in order])

    bad = [dict(mode=2), dict(mode=-1), dict(count=(1 << 31) + 1), dict(verdict=None), dict(ack=None),
           dict(replies=None), dict(total=None), dict(tmpl=None), dict(ack=good["ack"] + 2),
           dict(conn=good["conn"] + 1), dict(src=good["src"] + 3), dict(tmpl=good["tmpl"] + 8),
           dict(replies=good["replies"] + 4), dict(total=good["total"] + 4)]
    for kw in bad:
        assert call(**kw) == tcpck.EINVAL, kw
        assert (raw == 0xA5).all() and (src == 0xA5A5A5A5).all() and list(total) == [77, 77], kw
    # count == 0: nothing is needed but a valid mode, and the count comes back 0
    assert call(count=0, verdict=None, ack=None, conn=None, replies=None, src=None, tmpl=None, n_conns=0) == tcpck.OK
    assert total[0] == 0 and total[1] == 77
    assert call(count=0, total=None) == tcpck.OK and call(count=0, mode=5) == tcpck.EINVAL
    # 8-B offsets keep the u64 aligned, 4-B ones the u32 arrays
    assert call(total=good["total"] + 8, src=good["src"] + 4, replies=good["replies"] + 16) == tcpck.OK
    assert total[1] == reply_np(verdict, ack, conn, tmpl, 4, 50, 0)[2] and src[0] == 0xA5A5A5A5


def test_scratch_bytes(built_lib):
    import tcpck
    L = tcpck.lib()
    sizes = [tcpck.reply_scratch_bytes(n) for n in (0, 1, 1024, 1025, 1 << 20, (1 << 20) + 3, 1 << 31)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    out = ctypes.c_size_t(5)
    assert L.tcpck_reply_scratch_bytes((1 << 31) + 1, ctypes.byref(out)) == tcpck.EINVAL and out.value == 5
    assert L.tcpck_reply_scratch_bytes(8, None) == tcpck.EINVAL
