"""CPU tests of the multi-connection receive planner (tcpck_plan_deliver_multi)
and of the connection table's host mirror (tcpck_conn_table_*, host-only
tables).  The planner is held against tcpck_plan_deliver -- which
tests/test_deliver_plan.py pins to the reference's own records -- on every
connection's gathered subsequence, against tests/demux_np.py plan_multi_np, and
against the reference's records directly on the two golden sequences
interleaved in one ring.  No GPU call here."""
import ctypes

import numpy as np
import pytest

from deliver_np import SKIP, DeliverGolden, header_fields
from demux_np import (CONN_HOST, HOST, NONE, NOT_STOPPED, PORT_1, RST, STATE_KEYS, check_golden_ring, demux_np,
                      golden_ring, header_keys, mixed_ring, plan_multi_np)


def conn_state(tcpck, d):
    return tcpck.ConnState(tcpck.RcvState(d["rcv_nxt"], d["snd_nxt"], d["snd_una"], d["rcv_wnd"], 0, d["delivered"]),
                           d["recv_base"], d["recv_bytes"], 12345, d["flags"], 0)


@pytest.mark.parametrize("n_conns,per_conn,seed", [(1, 400, 1), (2, 300, 2), (7, 200, 3), (64, 60, 4)])
def test_multi_matches_the_single_planner_per_connection(built_lib, n_conns, per_conn, seed):
    import tcpck
    hdr, ok, lengths, conn, first = mixed_ring(seed, n_conns, per_conn)
    arr = (tcpck.ConnState * n_conns)(*[conn_state(tcpck, d) for d in first])
    dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, arr, lengths=lengths)
    # the numpy restatement walks the same ring
    model = [dict(d) for d in first]
    m_dst, m_verdict, m_ack = plan_multi_np(hdr, ok, conn, lengths, model)
    assert np.array_equal(dst, m_dst) and np.array_equal(verdict, m_verdict) and np.array_equal(ack, m_ack)
    rows = hdr.reshape(-1, 32)
    flags = header_fields(hdr)[3]
    reasons = set()
    for c in range(n_conns):
        at = np.flatnonzero(conn == c)
        st = tcpck.RcvState(*(first[c][k] for k in ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd")), 0, 0)
        s_dst, s_verdict, s_ack, consumed = tcpck.plan_deliver(rows[at].reshape(-1), ok[at], st, first[c]["recv_bytes"],
                                                               lengths=lengths[at])
        assert np.array_equal(verdict[at], s_verdict) and np.array_equal(ack[at], s_ack), c
        placed = s_dst != SKIP
        assert np.array_equal(dst[at][~placed], s_dst[~placed])
        assert np.array_equal(dst[at][placed], s_dst[placed] + np.uint64(first[c]["recv_base"])), c
        assert bytes(arr[c].rcv) == bytes(st), c
        assert arr[c].stopped_at == (at[consumed] if consumed < at.size else NOT_STOPPED), c
        assert {k: getattr(arr[c].rcv, k) for k in STATE_KEYS} == {k: model[c][k] for k in STATE_KEYS}
        assert arr[c].stopped_at == model[c]["stopped_at"]
        if consumed == at.size:
            reasons.add("ran")
        else:
            reasons.add("fin" if flags[at[consumed]] & 0x80 else "full")
    if n_conns >= 7:  # FINs in sequence mid-ring, windows that fill, walks that reach the end
        assert reasons == {"ran", "fin", "full"}
    if n_conns == 64:
        wrapped = [c for c in range(64) if arr[c].rcv.rcv_nxt < first[c]["rcv_nxt"]]
        assert wrapped, "no rcv_nxt passed 2^32"


def test_golden_ring_reproduces_the_reference(built_lib):
    """The fixture's two sequences as two connections interleaved in one ring: every per-image
    record of the reference, connection 1 stopping at its FIN while connection 0 runs on, the
    final control blocks."""
    import tcpck
    dg = DeliverGolden()
    ring = golden_ring(dg, tcpck.update16)
    hdr, ok = dg.host_headers(ring["wire"], ring["offsets"], ring["lengths"])
    # what the issue checked on the fixture: one key per sequence, damage included
    host_port, peer_ip, peer_port, _ = header_keys(hdr)
    keys = [set(zip(host_port[ring["which"] == c].tolist(), peer_ip[ring["which"] == c].tolist(),
                    peer_port[ring["which"] == c].tolist())) for c in (0, 1)]
    assert len(keys[0]) == len(keys[1]) == 1 and keys[0] != keys[1] and next(iter(keys[1]))[2] == PORT_1
    conn = demux_np(hdr, {next(iter(keys[0])): 0, next(iter(keys[1])): 1})
    assert np.array_equal(conn, ring["which"].astype(np.uint32))
    s0, s1 = dg.sequences
    guard = 64
    bases = (0, s0["recv_bytes"] + guard + (s0["recv_bytes"] & 1))
    for planner in ("library", "numpy"):
        first = [dict({k: s["initial"][k] for k in STATE_KEYS[:4]}, delivered=0, recv_base=b, recv_bytes=s["recv_bytes"],
                      flags=0) for s, b in zip(dg.sequences, bases)]
        if planner == "library":
            conns = (tcpck.ConnState * 2)(*[conn_state(tcpck, d) for d in first])
            dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=ring["lengths"])
        else:
            conns = first
            dst, verdict, ack = plan_multi_np(hdr, ok, conn, ring["lengths"], conns)
        check_golden_ring(dg, ring, hdr, ok, conn, dst, verdict, ack, conns)
    assert s1["left_estab_at"] >= 0 > s0["left_estab_at"]


def simple_ring(n, ports):
    """n in-order 100-B segments per listed source port (one connection each), round robin."""
    hdr = np.zeros((n * len(ports), 32), np.uint8)
    for k in range(hdr.shape[0]):
        i = k // len(ports)
        hdr[k, 10:12] = np.frombuffer((100).to_bytes(2, "little"), np.uint8)
        hdr[k, 12:14] = np.frombuffer(int(ports[k % len(ports)]).to_bytes(2, "little"), np.uint8)
        hdr[k, 16:20] = np.frombuffer((500 + 100 * i).to_bytes(4, "little"), np.uint8)
        hdr[k, 20:24] = np.frombuffer((7000 + k).to_bytes(4, "little"), np.uint8)
        hdr[k, 25] = 0x08
    return hdr.reshape(-1), np.ones(hdr.shape[0], np.uint8), np.full(hdr.shape[0], 132, np.uint32)


def fresh(tcpck, n, flags=()):
    d = [dict(rcv_nxt=500, snd_nxt=1 << 20, snd_una=0, rcv_wnd=0, delivered=0, recv_base=4096 * c, recv_bytes=4000,
              flags=(flags[c] if c < len(flags) else 0)) for c in range(n)]
    return (tcpck.ConnState * n)(*[conn_state(tcpck, x) for x in d]), d


def test_none_and_host_rules(built_lib):
    import tcpck
    hdr, ok, lengths = simple_ring(4, [1, 2, 3])  # 12 images: connections 0 (ESTAB), 1 (HOST), none
    conn = np.tile(np.asarray([0, 1, NONE], np.uint32), 4)
    ok[2] = 0   # unknown, bad sum, before any HOST image ... (k = 1 is already HOST: see below)
    ok[8] = 0
    # ring order 0, 1, NONE, ...: put an unknown image in front of the first HOST image
    order = np.asarray([2, 5, 0, 1, 3, 4, 6, 7, 8, 9, 10, 11])
    hdr, ok, lengths, conn = hdr.reshape(-1, 32)[order].reshape(-1), ok[order], lengths[order], conn[order]
    conns, model = fresh(tcpck, 2, flags=(0, tcpck.CONN_HOST))
    before_host = bytes(conns[1].rcv)
    dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=lengths)
    m = plan_multi_np(hdr, ok, conn, lengths, model)
    assert np.array_equal(dst, m[0]) and np.array_equal(verdict, m[1]) and np.array_equal(ack, m[2])
    acks = 7000 + order
    # ring slot 0: old image 2, bad sum, unknown -> nothing; slot 1: old image 5, good -> RST
    assert (verdict[0], ack[0], dst[0]) == (0, 0, SKIP)
    assert (verdict[1], ack[1], dst[1]) == (RST, acks[1], SKIP)
    host_slots = np.flatnonzero(conn == 1)
    assert (verdict[host_slots] == HOST).all() and (ack[host_slots] == 500).all() and (dst[host_slots] == SKIP).all()
    assert bytes(conns[1].rcv) == before_host and conns[1].stopped_at == NOT_STOPPED
    # unknown images after the first HOST image: good sum -> HOST, bad sum -> nothing
    later = [k for k in np.flatnonzero(conn == NONE) if k > host_slots[0]]
    assert len(later) == 2
    for k in later:
        assert (verdict[k], ack[k], dst[k]) == ((HOST, 0, SKIP) if ok[k] else (0, 0, SKIP))
    assert sorted(ok[later].tolist()) == [0, 1]
    # connection 0 is planned as ever, into its own window
    est = np.flatnonzero(conn == 0)
    assert (verdict[est] == 7).all() and dst[est].tolist() == [0, 100, 200, 300] and conns[0].rcv.delivered == 400
    assert (tcpck.RCV_RST, tcpck.RCV_HOST, tcpck.CONN_NONE, tcpck.NOT_STOPPED, tcpck.CONN_HOST, tcpck.CONN_ESTAB) == (
        RST, HOST, NONE, NOT_STOPPED, CONN_HOST, 0)
    # a HOST image with a bad sum is still the host's, and n_conns == 0 takes an all-unknown ring
    ok[host_slots[0]] = 0
    conns, _ = fresh(tcpck, 2, flags=(0, tcpck.CONN_HOST))
    assert tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=lengths)[1][host_slots[0]] == HOST
    none = np.full(conn.size, NONE, np.uint32)
    dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, none, (tcpck.ConnState * 0)(), lengths=lengths)
    assert (verdict == np.where(ok, RST, 0)).all() and (ack == np.where(ok, acks, 0)).all() and (dst == SKIP).all()


def test_stopped_connection_leaves_the_others_running(built_lib):
    import tcpck
    hdr, ok, lengths = simple_ring(10, [1, 2])
    conn = np.tile(np.asarray([0, 1], np.uint32), 10)
    conns, _ = fresh(tcpck, 2)
    conns[0].recv_bytes = 350  # room for three payloads
    conns[1].rcv.delivered = 2
    dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=lengths)
    assert conns[0].stopped_at == 6 and conns[1].stopped_at == NOT_STOPPED
    assert dst[0::2].tolist() == [0, 100, 200] + [SKIP] * 7 and (verdict[6::2] == 0).all() and (ack[6::2] == 800).all()
    assert dst[1::2].tolist() == [4096 + 2 + 100 * i for i in range(10)] and conns[1].rcv.delivered == 1002
    # a list of ConnState is updated in place too
    as_list = list(fresh(tcpck, 2)[0])
    tcpck.plan_deliver_multi(hdr, ok, conn, as_list, lengths=lengths)
    assert as_list[0].rcv.delivered == 1000 and as_list[0].stopped_at == NOT_STOPPED


def test_argument_errors(built_lib):
    import tcpck
    L = tcpck.lib()
    hdr, ok, lengths = simple_ring(3, [1, 2])
    n = ok.size
    conn = np.tile(np.asarray([0, 1], np.uint32), 3)
    dst, ver, ack = np.full(n, 0x5A5A, np.uint64), np.full(n, 0x5A, np.uint8), np.full(n, 0x5A5A, np.uint32)

    def call(conns, **change):
        a = dict(hdr=hdr.ctypes.data, ok=ok.ctypes.data, conn=conn.ctypes.data, lengths=lengths.ctypes.data, len=0,
                 count=n, conns=conns, n_conns=len(conns) if conns is not None else 2, dst=dst.ctypes.data,
                 ver=ver.ctypes.data, ack=ack.ctypes.data)
        a.update(change)
        return L.tcpck_plan_deliver_multi(a["hdr"], a["ok"], a["conn"], a["lengths"], a["len"], a["count"], a["conns"],
                                          a["n_conns"], a["dst"], a["ver"], a["ack"])

    def untouched(conns):
        assert (dst == 0x5A5A).all() and (ver == 0x5A).all() and (ack == 0x5A5A).all()
        assert all(c.stopped_at == 12345 and c.rcv.delivered == conns_first[i] for i, c in enumerate(conns))

    conns_first = [0, 0]
    for name in ("hdr", "ok", "conn", "dst", "ver", "ack"):  # each pointer NULL in turn (h_lengths may be)
        conns, _ = fresh(tcpck, 2)
        assert call(conns, **{name: None}) == tcpck.EINVAL, name
        untouched(conns)
    conns, _ = fresh(tcpck, 2)
    assert call(None) == tcpck.EINVAL
    for length in (0, 30, 33, 65):  # h_lengths NULL: `len` short or odd
        assert call(conns, lengths=None, len=length) == tcpck.EINVAL, length
    for v in (30, 33, 0):
        bad = lengths.copy()
        bad[n - 1] = v
        assert call(conns, lengths=bad.ctypes.data) == tcpck.EINVAL, v
    for v in (2, 3, NONE - 1):  # neither NONE nor below n_conns
        bad = conn.copy()
        bad[n - 1] = v
        assert call(conns, conn=bad.ctypes.data) == tcpck.EINVAL, v
    assert call(conns, n_conns=1) == tcpck.EINVAL
    untouched(conns)
    for field, value in (("recv_base", 4097), ("recv_base", (1 << 64) - 2), ("recv_bytes", (1 << 64) - 4096)):
        conns, _ = fresh(tcpck, 2)
        setattr(conns[1], field, value)
        assert call(conns) == tcpck.EINVAL, (field, value)
        untouched(conns)
    conns, _ = fresh(tcpck, 2)
    conns[1].rcv.delivered = 4001
    conns_first = [0, 4001]
    assert call(conns) == tcpck.EINVAL
    untouched(conns)
    # the same arguments unbroken are fine; so are no images and no connections at all
    conns_first = [0, 0]
    conns, _ = fresh(tcpck, 2)
    assert call(conns) == tcpck.OK and (ver == 7).all()
    assert call(conns, lengths=None, len=132) == tcpck.OK
    assert L.tcpck_plan_deliver_multi(None, None, None, None, 0, 0, None, 0, None, None, None) == tcpck.OK
    assert L.tcpck_plan_deliver_multi(None, None, None, None, 0, 0, conns, 2, None, None, None) == tcpck.OK
    assert conns[0].stopped_at == NOT_STOPPED
    with pytest.raises(ValueError):
        tcpck.plan_deliver_multi(hdr, ok, conn[:-1], conns, lengths=lengths)
    assert ctypes.sizeof(tcpck.ConnState) == 56


# ---- the connection table's host mirror ---------------------------------------

def test_table_set_overwrite_erase_find_full(built_lib):
    import tcpck
    L = tcpck.lib()
    with tcpck.ConnTable(None, 3) as t:
        assert t.find(80, 0, 0) == NONE
        t.set(80, 0, 0, 7)                    # a listener
        t.set(80, 0x0A000001, 4000, 8)
        t.set(80, 0x0A000001, 4001, 0)
        assert (t.find(80, 0, 0), t.find(80, 0x0A000001, 4000), t.find(80, 0x0A000001, 4001)) == (7, 8, 0)
        for miss in ((81, 0, 0), (80, 0x0A000002, 4000), (80, 0x0A000001, 4002), (4000, 0x0A000001, 80)):
            assert t.find(*miss) == NONE  # equality is exact on every field
        t.set(80, 0x0A000001, 4000, 9)        # overwrite: no new entry
        assert t.find(80, 0x0A000001, 4000) == 9
        with pytest.raises(tcpck.TcpckError) as e:
            t.set(81, 0, 0, 1)                # a fourth key
        assert e.value.status == tcpck.ENOMEM
        assert (t.find(81, 0, 0), t.find(80, 0, 0), t.find(80, 0x0A000001, 4000)) == (NONE, 7, 9)
        t.set(80, 0, 0, 70)                   # a full table still overwrites
        with pytest.raises(tcpck.TcpckError) as e:
            t.set(80, 0, 0, NONE)
        assert e.value.status == tcpck.EINVAL and t.find(80, 0, 0) == 70
        t.erase(80, 0, 0)
        t.erase(80, 0, 0)                     # absent: fine
        t.erase(9, 9, 9)
        assert t.find(80, 0, 0) == NONE
        t.set(81, 0, 0, 1)                    # room again
        assert t.stats() == (0, 0, 0, 0)      # nothing committed yet
        t.commit()                            # host only: the image is rebuilt, nothing uploaded
        slots, entries, longest, wrapped = t.stats()
        assert (slots, entries) == (64, 3) and 1 <= longest <= 3 and wrapped <= 3
        t.erase(81, 0, 0)
        assert t.stats()[1] == 3              # ... of the committed image, not the mirror
        # NULL out-pointers, NULL tables, the size bounds
        assert L.tcpck_conn_table_stats(t._h, None, None, None, None) == tcpck.OK
        assert L.tcpck_conn_table_find(t._h, 1, 1, 1, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(None, t._h, None, 0, None, None) == tcpck.EINVAL
    for f, args in ((L.tcpck_conn_table_set, (1, 1, 1, 1)), (L.tcpck_conn_table_erase, (1, 1, 1)),
                    (L.tcpck_conn_table_find, (1, 1, 1, ctypes.byref(ctypes.c_uint32()))),
                    (L.tcpck_conn_table_commit, (None,)), (L.tcpck_conn_table_stats, (None, None, None, None)),
                    (L.tcpck_conn_table_destroy, ())):
        assert f(None, *args) == tcpck.EINVAL
    h = ctypes.c_void_p()
    for bad in (0, (1 << 22) + 1):
        assert L.tcpck_conn_table_create(None, bad, ctypes.byref(h)) == tcpck.EINVAL
    assert L.tcpck_conn_table_create(None, 4, None) == tcpck.EINVAL
    with tcpck.ConnTable(None, 33) as t:      # slots: a power of two >= 2 * max_conns, at least 64
        t.commit()
        assert t.stats()[0] == 128


def test_table_churn_against_a_dict(built_lib):
    """5,000 seeded operations over 300 clustered keys in a table of 128: set (new, overwrite,
    refused when full), erase (present, absent), find -- the mirror agrees with a dict all along,
    and so does a committed image's entry count."""
    import tcpck
    rng = np.random.default_rng(17)
    keys = [(80 + i % 3, 0x0A000000 + i // 6, 4000 + i % 6) for i in range(297)] + [(80, 0, 0), (81, 0, 0), (82, 0, 0)]
    want, refused, erased = {}, 0, 0
    with tcpck.ConnTable(None, 128) as t:
        for step in range(5000):
            key = keys[int(rng.integers(0, len(keys)))]
            r = rng.random()
            if r < 0.5:
                id_ = int(rng.integers(0, 1 << 32)) % NONE
                if key in want or len(want) < 128:
                    t.set(*key, id_)
                    want[key] = id_
                else:
                    with pytest.raises(tcpck.TcpckError) as e:
                        t.set(*key, id_)
                    assert e.value.status == tcpck.ENOMEM
                    refused += 1
            elif r < 0.8:
                erased += key in want
                t.erase(*key)
                want.pop(key, None)
            assert t.find(*key) == want.get(key, NONE), step
            if step % 500 == 499:
                assert all(t.find(*k) == want.get(k, NONE) for k in keys), step
                t.commit()
                assert t.stats()[:2] == (256, len(want))
    assert refused > 20 and erased > 500 and len(want) > 100
