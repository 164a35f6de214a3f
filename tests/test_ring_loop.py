"""The receive loop on the CPU: tests/ring_loop.py's numpy backend to the end of every stream, and
beside it, on the same rings, the library's host twins -- tcpck.plan_deliver_multi against
plan_multi_np (arrays and every tcpck_conn_state field), tcpck.build_replies against reply_np, a
host-only connection table against the dict after every control-plane step, tcpck.checksum16 on
every reply -- with state carried from ring to ring.  The scenario has to reach what it claims
to reach: the coverage assertions keep a later edit from quietly emptying it."""
import numpy as np
import pytest

import ring_loop
from demux_np import NONE
from ring_loop import RING_COUNT, LibTwin, NumpyBackend, Scenario, compare, run


def twin_ring(twin, mode):
    import tcpck

    def per_ring(loop, R, outs, steps):
        want = outs[0]
        if steps or loop.r == 0:  # the table's host mirror against the dict, key by key
            keys = [loop.key(c) for c in range(loop.scn.n_conns)] + [(ring_loop.LISTEN_PORT, 0, 0), (1, 2, 3)]
            for key in keys:
                assert twin.table.find(*key) == loop.backends[0].table.get(key, NONE), (loop.r, key)
        got = twin.ring(R, want)
        compare(loop.r, got, want, keys=("dst", "verdict", "ack"))
        total = int(want["count"][0])
        assert got["total"] == total
        assert np.array_equal(got["rows"].reshape(-1), want["replies"][:32 * total])
        assert np.array_equal(got["src"], want["src"][:total])
        for row in got["rows"]:
            assert tcpck.checksum16(row, mode) == 0

    return per_ring


@pytest.fixture(scope="module", params=[(0, 0), (1, 0), (0, 1), (1, 1)], ids=lambda p: f"mode{p[0]}-seed{p[1]}")
def finished(request, built_lib):
    """One loop run to its end: numpy backend first (the sender reads its replies), the twins beside it."""
    mode, seed = request.param
    scn = Scenario(seed, mode)
    twin = LibTwin(scn, mode)
    return run(scn, [NumpyBackend(scn, mode), twin], twin_ring(twin, mode)), seed


def test_streams_arrive_and_the_ring_count_is_the_recorded_one(finished):
    loop, seed = finished  # run() made the end-of-loop checks
    assert loop.r == RING_COUNT[(seed, 2)] == loop.scn.rings < ring_loop.HARD_STOP


def test_the_scenario_reaches_what_it_claims(finished):
    loop, _ = finished
    cov, scn = loop.cov, loop.scn
    for kind in ("dropped", "duplicated", "swapped", "damaged"):
        assert min(cov[kind]) >= 1, (kind, cov[kind])
    assert cov["full_drains"] >= 1 and cov["resumed"] >= 1
    assert cov["fin_stops"] >= 1 and cov["fin_host"] >= 1
    assert cov["listener_host"] >= 2 and cov["unknown_host"] >= 2 and cov["unknown_rst"] >= 1
    assert cov["rst_before_set"] == ring_loop.LATE_SET_RING and cov["rst_after_erase"] == ring_loop.RST_RINGS_BEFORE_ABORT
    assert cov["bad_ack_rejected"] >= 1
    assert max(loop.rewrites.values()) >= 3
    b = loop.backends[0]
    for c, cn in enumerate(scn.conns):
        end = b.get_state(loop.cid[c])["rcv_nxt"]
        if cn["role"].startswith("wrap32"):
            assert end < cn["iss"] < 1 << 32, "the sequence number did not wrap"
        if cn["role"] == "cross31":
            assert cn["iss"] < 1 << 31 <= end
    assert any(cn["lens"][-1] == 34 for cn in scn.conns)


def test_eleven_connections(built_lib):
    """The second scenario of the two-loop device test (another seed, one connection more)."""
    scn = Scenario(2, 0, plain=3)
    twin = LibTwin(scn, 0)
    loop = run(scn, [NumpyBackend(scn, 0), twin], twin_ring(twin, 0))
    assert loop.r == RING_COUNT[(2, 3)] and scn.n_conns == 11 and 1024 < max(loop.sizes) <= ring_loop.MAX_RING


def test_ring_sizes(finished):
    loop, _ = finished
    sizes = loop.sizes
    assert max(sizes) > 1024 and max(sizes) <= ring_loop.MAX_RING
    assert any(s % 64 for s in sizes)
    assert min(sizes[-3:]) < 64
