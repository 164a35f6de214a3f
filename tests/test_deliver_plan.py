"""CPU tests of the receive delivery planner (tcpck_plan_deliver) and the numpy
restatements in tests/deliver_np.py, against tests/golden/deliver_golden.* --
what the reference's TcpStateManager in Estab (state.cc:195-223) and
SocketInternal::Accept()'s append (socket-internal.h:323-334) did with two
arrival sequences (tests/golden/gen_deliver.cc).  No GPU call here."""
import ctypes

import numpy as np
import pytest

from deliver_np import (ACCEPT, BAD_SUM, PAYLOAD, SEND_ACK, SKIP, DeliverGolden, deliver_np, plan_np,
                        random_arrivals)

STATE_KEYS = ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd")


@pytest.fixture(scope="module")
def dg():
    return DeliverGolden()


def make_state(tcpck, d, delivered=0):
    return tcpck.RcvState(d["rcv_nxt"], d["snd_nxt"], d["snd_una"], d["rcv_wnd"], 0, delivered)


def state_dict(st):
    return {k: getattr(st, k) for k in STATE_KEYS + ("delivered",)}


def plan_c(tcpck, hdr, ok, lengths, state, recv_bytes):
    st = make_state(tcpck, state, state["delivered"])
    dst, verdict, ack, consumed = tcpck.plan_deliver(hdr, ok, st, recv_bytes, lengths=lengths)
    state.update(state_dict(st))
    return dst, verdict, ack, consumed


def planners(built_lib):
    import tcpck
    return {"numpy": plan_np, "library": lambda *a: plan_c(tcpck, *a)}


@pytest.mark.parametrize("which", ["numpy", "library"])
def test_planner_reproduces_the_reference(dg, built_lib, which):
    plan = planners(built_lib)[which]
    assert sum(len(s["offsets"]) for s in dg.sequences) >= 100
    assert any(s["left_estab_at"] >= 0 for s in dg.sequences) and any(s["left_estab_at"] < 0 for s in dg.sequences)
    for s in dg.sequences:
        wire = dg.wire(s)
        n = len(s["offsets"])
        hdr, ok = dg.host_headers(wire, s["offsets"], s["lengths"])
        assert ok.tolist() == s["ok"]
        state = dict({k: s["initial"][k] for k in STATE_KEYS}, delivered=0)
        dst, verdict, ack, consumed = plan(hdr, ok, np.asarray(s["lengths"], np.uint32), state, s["recv_bytes"])
        stop = s["left_estab_at"] if s["left_estab_at"] >= 0 else n
        assert consumed == stop
        at = 0
        for k in range(n):
            if k >= stop:  # the FIN in sequence: left to the state machine
                assert s["accepted"][k] == 1 and verdict[k] == 0 and dst[k] == SKIP
                continue
            want = 0
            if not s["ok"][k]:
                want = BAD_SUM | SEND_ACK
                assert s["discarded"][k] == 1 and s["send_ack"][k] == 1 and s["accepted"][k] == 0
            elif s["accepted"][k]:
                want = ACCEPT | (SEND_ACK if s["send_ack"][k] else 0) | (PAYLOAD if s["appended"][k] else 0)
                assert s["recv_ack"][k] == 1
            else:
                assert s["discarded"][k] == 1 and s["send_ack"][k] == 0
            assert verdict[k] == want, (k, verdict[k], want)
            if s["send_ack"][k]:
                assert ack[k] == s["reply_ack"][k] and s["reply_seq"][k] == s["initial"]["snd_nxt"], k
            if s["appended"][k]:
                assert dst[k] == at and s["appended"][k] == s["lengths"][k] - 32
                at += s["appended"][k]
            else:
                assert dst[k] == SKIP
        assert at == s["recv_bytes"] == state["delivered"]
        assert {k: state[k] for k in STATE_KEYS} == {k: s["final"][k] for k in STATE_KEYS}
        # Accept()'s appends as a scatter: the reference's recv_buffer
        recv = deliver_np(wire, s["offsets"], s["lengths"], dst, np.full(s["recv_bytes"], 0xA5, np.uint8))
        assert np.array_equal(recv, dg.recv(s))


def test_golden_pins_the_append_of_the_whole_buffer(dg):
    """The reference appends begin()..end() -- len - 32 bytes -- whatever TcpLength says, and nothing
    for an empty payload even when TcpLength > 0; both cases and a seq wrap are in the fixture."""
    from deliver_np import header_fields
    seen = set()
    for s in dg.sequences:
        hdr, _ = dg.host_headers(dg.wire(s), s["offsets"], s["lengths"])
        tl = header_fields(hdr)[0]
        for k, ln in enumerate(s["lengths"]):
            if s["accepted"][k] and s["ok"][k] and k != s["left_estab_at"]:
                if tl[k] and tl[k] != ln - 32:
                    seen.add("shorter" if tl[k] < ln - 32 else ("empty" if ln == 32 else "longer"))
                    assert s["appended"][k] == ln - 32
        if s["final"]["rcv_nxt"] < s["initial"]["rcv_nxt"]:
            seen.add("wrap")
    assert seen == {"shorter", "longer", "empty", "wrap"}


@pytest.mark.parametrize("seed,rcv_nxt", [(1, 1000), (2, 0xFFFFFFFF - 40000), (3, 0x7FFFFFF0)])
def test_planner_matches_numpy_on_random_arrivals(built_lib, seed, rcv_nxt):
    import tcpck
    rng = np.random.default_rng(seed)
    base = dict(rcv_nxt=rcv_nxt, snd_nxt=5000, snd_una=4990, rcv_wnd=7, delivered=0)
    hdr, ok, lengths = random_arrivals(rng, 3000, base)
    at, rounds = 0, 0
    a, b = dict(base), dict(base)
    while at < ok.size:  # a FIN in sequence stops the walk: step over it and go on
        sl = slice(at, ok.size)
        ra = plan_np(hdr[32 * at:], ok[sl], lengths[sl], a, 1 << 40)
        rb = plan_c(tcpck, hdr[32 * at:], ok[sl], lengths[sl], b, 1 << 40)
        for x, y in zip(ra[:3], rb[:3]):
            assert np.array_equal(x, y)
        assert ra[3] == rb[3] and a == b
        at += ra[3] + 1
        rounds += 1
    assert rounds > 3 and a["delivered"] > 100000 and a["snd_una"] == 5000


def test_capacity_stop(built_lib):
    import tcpck
    n = 20
    hdr = np.zeros((n, 32), np.uint8)
    for k in range(n):
        hdr[k, 10:12] = np.frombuffer((100).to_bytes(2, "little"), np.uint8)
        hdr[k, 16:20] = np.frombuffer((500 + 100 * k).to_bytes(4, "little"), np.uint8)
        hdr[k, 25] = 0x08
    lengths = np.full(n, 132, np.uint32)
    ok = np.ones(n, np.uint8)
    for cap, fit in ((1000, 10), (1099, 10), (999, 9), (0, 0), (2000, 20), (5000, 20)):
        for plan in (plan_np, lambda *a: plan_c(tcpck, *a)):
            st = dict(rcv_nxt=500, snd_nxt=9, snd_una=0, rcv_wnd=0, delivered=0)
            dst, verdict, ack, consumed = plan(hdr.reshape(-1), ok, lengths, st, cap)
            assert consumed == fit and st["delivered"] == 100 * fit and st["rcv_nxt"] == 500 + 100 * fit
            assert (dst[:fit] == np.arange(fit) * 100).all() and (dst[fit:] == SKIP).all()
            assert (verdict[:fit] == (ACCEPT | PAYLOAD | SEND_ACK)).all() and (verdict[fit:] == 0).all()
            assert (ack[fit:] == st["rcv_nxt"]).all()
    # an image without payload passes a full stream
    hdr[0, 10:12] = 0
    st = dict(rcv_nxt=500, snd_nxt=9, snd_una=0, rcv_wnd=0, delivered=0)
    dst, verdict, ack, consumed = plan_c(tcpck, hdr.reshape(-1)[:32], ok[:1], np.asarray([32], np.uint32), st, 0)
    assert consumed == 1 and verdict[0] == ACCEPT and dst[0] == SKIP


def test_argument_errors(built_lib):
    import tcpck
    L = tcpck.lib()
    n = 4
    hdr = np.zeros(32 * n, np.uint8)
    ok = np.ones(n, np.uint8)
    ln = np.full(n, 64, np.uint32)
    dst, ver, ack = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    st, used = tcpck.RcvState(), ctypes.c_uint64()
    good = [hdr.ctypes.data, ok.ctypes.data, ln.ctypes.data, 0, n, ctypes.byref(st), 1 << 20, dst.ctypes.data,
            ver.ctypes.data, ack.ctypes.data, ctypes.byref(used)]
    assert L.tcpck_plan_deliver(*good) == tcpck.OK
    for i in (0, 1, 5, 7, 8, 9, 10):  # each pointer NULL in turn (h_lengths may be)
        bad = list(good)
        bad[i] = None
        assert L.tcpck_plan_deliver(*bad) == tcpck.EINVAL, i
    for length in (0, 30, 33, 65):  # h_lengths NULL: `len` short or odd
        bad = list(good)
        bad[2], bad[3] = None, length
        assert L.tcpck_plan_deliver(*bad) == tcpck.EINVAL, length
    bad = list(good)
    bad[2], bad[3] = None, 64
    assert L.tcpck_plan_deliver(*bad) == tcpck.OK
    for v in (30, 33, 0):
        ln2 = ln.copy()
        ln2[2] = v
        bad = list(good)
        bad[2] = ln2.ctypes.data
        assert L.tcpck_plan_deliver(*bad) == tcpck.EINVAL, v
    with pytest.raises(ValueError):
        tcpck.plan_deliver(hdr[:-1], ok, st, 100, lengths=ln)
    # tcpck_batch_deliver: the checks that come before any device call
    assert L.tcpck_batch_deliver(None, 16, 64, 64, None, None, 1, 16, 16, 64, None) == tcpck.EINVAL
    assert tcpck.DELIVER_SKIP == SKIP and (tcpck.RCV_ACCEPT, tcpck.RCV_PAYLOAD, tcpck.RCV_SEND_ACK, tcpck.RCV_BAD_SUM) == (
        ACCEPT, PAYLOAD, SEND_ACK, BAD_SUM)
    assert ctypes.sizeof(tcpck.RcvState) == 24


def _small_cases():
    from deliver_cases import (alignment_case, guard_rails_cases, jumbo_cases, random_rule_case, scattered_case,
                               shapes_cases)
    cases = [alignment_case(6, 0), alignment_case(10, 2), scattered_case(), random_rule_case(4000, 71)]
    cases += guard_rails_cases() + jumbo_cases(9000, 7) + jumbo_cases(65536, 5)
    for layout in ("fixed", "slots", "packed"):
        cases += shapes_cases(65, layout) + shapes_cases(257, layout)
    return cases


def test_deliver_np_fast_is_the_loop_form():
    """deliver_np_fast (the vectorised form the large GPU tests compare with) byte for byte against
    deliver_np, on the inputs of the small GPU tests and on 4000 random images of which a third
    break one clause of the skip rule each; small `chunk` values put the round boundaries of the
    gather inside the batch."""
    from deliver_np import deliver_np_fast
    cases = _small_cases()
    rule = cases[3]
    ln, off, d = (np.asarray(v).astype(np.uint64) for v in (rule.lengths, rule.offsets, rule.dst))
    # every clause is present among the random images, and so are delivered ones
    assert (ln & 1).any() and (off & 1).any() and (ln < 32).any() and (ln == 32).any() and (ln > 1 << 24).any()
    assert ((d & 1) == 1).sum() > (d == SKIP).sum() > 0 and (d[d != SKIP] > rule.recv_bytes).any()
    for c in cases:
        alloc = c.recv_bytes if c.recv_alloc is None else c.recv_alloc
        want = np.full(alloc, 0xA5, np.uint8)
        deliver_np(c.arena, c.offsets, c.lengths, c.dst, want[:c.recv_bytes])
        for chunk in (1 << 22, 4096, 1):
            got = np.full(alloc, 0xA5, np.uint8)
            deliver_np_fast(c.arena, c.offsets, c.lengths, c.dst, got[:c.recv_bytes], chunk=chunk)
            assert np.array_equal(got, want), chunk
    assert (want != 0xA5).any()


def test_deliver_np_skip_rule():
    """Each clause of include/tcpck.h's skip rule on its own, in both forms: nothing lands."""
    from deliver_np import deliver_np_fast
    arena = np.arange(4096, dtype=np.uint8)
    bad = [(0, 101, 0), (1, 100, 0), (0, 30, 0), (0, 0, 0), (0, 32, 0), (0, (1 << 24) + 2, 0), (0, 0xFFFFFFFE, 0),
           (0, 100, 1), (0, 100, SKIP), (0, 100, 190), (0, 100, (1 << 64) - 2)]
    for form in (deliver_np, deliver_np_fast):
        for off, ln, d in bad:
            recv = form(arena, [off, 256], [ln, 40], [d, 100], np.full(256, 0xA5, np.uint8))
            want = np.full(256, 0xA5, np.uint8)
            want[100:108] = arena[288:296]
            assert np.array_equal(recv, want), (form.__name__, off, ln, d)
        recv = form(arena, [0], [100], [188], np.full(256, 0xA5, np.uint8))  # ends exactly at the end
        assert np.array_equal(recv[188:], arena[32:100]) and (recv[:188] == 0xA5).all()
