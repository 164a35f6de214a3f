"""The receive loop on the device: tests/ring_loop.py's DeviceBackend (tcpck_batch_segment,
tcpck_batch_set_ack, tcpck_batch_receive, tcpck_batch_demux, tcpck_plan_deliver_multi on a
persistent tcpck_conn_state array, tcpck_batch_deliver into one shared buffer, tcpck_batch_reply)
and the numpy backend advance ring by ring on identical rings; the sender reads the DEVICE's reply
bytes.  After every ring whole arrays are compared -- the arena after the ACK rewrite, d_ok, the
header array, d_conn, the planner's outputs on the device's own inputs and every state field, the
shared receive buffer with its sentinels, the reply ring, d_src and d_count with their guard
elements, the scratch's guard -- and at the end every receive stream is its send stream."""
import time

import pytest

from ring_loop import DeviceBackend, Loop, NumpyBackend, Scenario, compare, run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available()
    c = tcpck.Context(0)
    yield c
    c.close()


def torch_allocations():
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def lockstep(loop, R, outs, steps):
    compare(loop.r, outs[0], outs[1])


def run_loop(ctx, mode, seed, stream=None, before_ring=None):
    scn = Scenario(seed, mode)
    dev = DeviceBackend(scn, mode, ctx, stream)
    try:
        t0, allocated = time.perf_counter(), torch_allocations()
        loop = run(scn, [dev, NumpyBackend(scn, mode)], before_ring or lockstep, want_rings=scn.rings)
        assert torch_allocations() == allocated, "the loop allocated device memory"
        print(f"mode {mode} seed {seed}: {loop.r} rings, {sum(loop.sizes)} images, {time.perf_counter() - t0:.2f} s")
    finally:
        dev.close()
    return loop


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_device_loop_against_the_model(ctx, mode, seed):
    run_loop(ctx, mode, seed)


def test_device_loop_on_a_side_stream(ctx):
    """Every device call on a non-default stream; per ring no synchronisation but the copy down the
    planner needs and the read-back the comparisons need."""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_loop(ctx, 1, 1, stream=s)


def test_two_loops_two_streams_one_context(ctx):
    """Two loops that differ in seed, connections, mode, table, buffers and scratch share one
    context and run on two streams, interleaved call by call; each is checked as above."""
    specs = [(Scenario(0, 0), 0), (Scenario(2, 1, plain=3), 1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    devs = [DeviceBackend(scn, mode, ctx, s) for (scn, mode), s in zip(specs, streams)]
    try:
        loops = [Loop(scn, [dev, NumpyBackend(scn, mode)]) for (scn, mode), dev in zip(specs, devs)]
        for lp in loops:
            lp.start()
        allocated = torch_allocations()
        while True:
            live = [lp for lp in loops if not lp.done()]
            if not live:
                break
            rings = []
            for lp in live:
                assert lp.r < 200
                lp.control()
                rings.append(lp.begin_ring())
            steps = [lp.backends[0].ring_steps(R) for lp, R in zip(live, rings)]
            while steps:  # one call of each loop in turn
                for g in list(steps):
                    if next(g, "end") == "end":
                        steps.remove(g)
            for lp, R in zip(live, rings):
                got = lp.backends[0].out
                compare(lp.r, got, lp.backends[1].ring(R))
                lp.end_ring(R, got)
        assert torch_allocations() == allocated, "the loops allocated device memory"
        for lp in loops:
            assert lp.r == lp.scn.rings
            for b in lp.backends:
                lp.final_checks(b)
    finally:
        for d in devs:
            d.close()


def test_captured_second_half_replays_every_ring(ctx):
    """tcpck_batch_deliver + tcpck_batch_reply promise `nothing is allocated; no host
    synchronisation`: after an uncaptured first ring both are captured once, on one stream (a
    linear chain), over fixed buffers and the scenario's largest ring as the count; every later
    ring copies its dst, verdict, ack and conn into those buffers -- shorter rings padded with
    SKIP destinations and verdict 0 -- and replays.  The same whole-array comparisons per ring,
    the same checks at the end."""
    mode, seed = 0, 0
    scn = Scenario(seed, mode)
    largest = max(run(scn, [NumpyBackend(scn, mode)]).sizes)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev = DeviceBackend(scn, mode, ctx, s)
    replayed = []

    def per_ring(loop, R, outs, steps):
        compare(loop.r, outs[0], outs[1])
        replayed.append(dev.graph is not None)
        if loop.r == 0:
            dev.capture(largest)

    try:
        loop = run(scn, [dev, NumpyBackend(scn, mode)], per_ring, want_rings=scn.rings)
        assert replayed == [False] + [True] * (loop.r - 1) and max(loop.sizes) == largest > min(loop.sizes)
    finally:
        dev.close()
