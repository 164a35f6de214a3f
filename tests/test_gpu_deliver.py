"""GPU tests of tcpck_batch_deliver: the accepted payloads of a receive batch
copied into the receive stream (SocketInternal::Accept()'s append,
include/socket-internal.h:323-334), against the reference's own recv_buffer
(tests/golden/deliver_golden.*, tests/golden/gen_deliver.cc) and against the
numpy restatement tests/deliver_np.py.  Every case pre-fills the receive buffer
with 0xA5 and compares it WHOLE, so a byte written outside a delivered range
fails."""
import numpy as np
import pytest

from deliver_cases import (alignment_case, back_to_back, guard_rails_cases, jumbo_cases, scattered_case,
                           shapes_cases)
from deliver_np import SKIP, DeliverGolden, deliver_np, plan_np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available()
    c = tcpck.Context(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(ctx, arena, offsets, lengths, dst, recv_bytes, fixed=None, recv_alloc=None, stream=None, base_mis=0,
          count=None):
    """Delivers on the device and compares the whole receive buffer (recv_alloc >= recv_bytes
    bytes of it, the rest guard) with deliver_np; returns it.  base_mis: the arena starts that
    many bytes into its allocation.  count: only the first `count` images are the batch -- the
    device arrays still hold them all, and the others must leave no trace."""
    offsets = np.asarray(offsets, np.uint64)
    lengths = np.asarray(lengths, np.uint32)
    dst = np.asarray(dst, np.uint64)
    count = len(dst) if count is None else count
    recv_alloc = recv_bytes if recv_alloc is None else recv_alloc
    d_arena = torch.zeros(base_mis + arena.size + (16 if base_mis else 0), dtype=torch.uint8, device="cuda")
    d_arena = d_arena[base_mis:base_mis + arena.size]  # (a view: the allocation lives as long as it does)
    d_arena.copy_(torch.from_numpy(np.ascontiguousarray(arena)))
    d_recv = torch.full((max(recv_alloc, 16),), FILL, dtype=torch.uint8, device="cuda")
    d_dst = dev(dst)
    torch.cuda.synchronize()  # the uploads and the fill ran on torch's stream
    p_arena = d_arena.data_ptr() if base_mis else d_arena
    if fixed:
        stride, length = fixed
        ctx.batch_deliver(p_arena, count, d_dst, d_recv, recv_bytes, stride=stride, length=length, stream=stream)
    else:
        d_off, d_len = dev(offsets), dev(lengths)
        torch.cuda.synchronize()
        ctx.batch_deliver(p_arena, count, d_dst, d_recv, recv_bytes, offsets=d_off, lengths=d_len, stream=stream)
    got = host(d_recv)
    want = np.full(got.size, FILL, np.uint8)
    deliver_np(arena, offsets[:count], lengths[:count], dst[:count], want[:recv_bytes])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    assert np.array_equal(host(d_arena), arena), "the arena is read only"
    return got


def run(ctx, case, **kw):
    """check() on a deliver_cases.Case."""
    return check(ctx, case.arena, case.offsets, case.lengths, case.dst, case.recv_bytes, fixed=case.fixed,
                 recv_alloc=case.recv_alloc, **kw)


def test_golden_receive_plan_deliver(ctx):
    """Wire arena -> batch_receive -> plan_deliver -> batch_deliver == the reference's recv_buffer."""
    import tcpck
    dg = DeliverGolden()
    for s in dg.sequences:
        wire = dg.wire(s)
        n = len(s["offsets"])
        offsets, lengths = np.asarray(s["offsets"], np.uint64), np.asarray(s["lengths"], np.uint32)
        d_wire, d_off, d_len = dev(wire), dev(offsets), dev(lengths)
        ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        hdr = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        ctx.batch_receive(d_wire, n, ok, hdr, offsets=d_off, lengths=d_len)
        st = tcpck.RcvState(*(s["initial"][k] for k in ("rcv_nxt", "snd_nxt", "snd_una", "rcv_wnd")), 0, 0)
        dst, verdict, ack, consumed = tcpck.plan_deliver(host(hdr), host(ok), st, s["recv_bytes"], lengths=lengths)
        assert consumed == (s["left_estab_at"] if s["left_estab_at"] >= 0 else n)
        assert st.delivered == s["recv_bytes"] and st.rcv_nxt == s["final"]["rcv_nxt"]
        d_recv = torch.full((s["recv_bytes"] + 64,), FILL, dtype=torch.uint8, device="cuda")
        ctx.batch_deliver(d_wire, n, dev(dst), d_recv, s["recv_bytes"], offsets=d_off, lengths=d_len)
        got = host(d_recv)
        assert np.array_equal(got[:s["recv_bytes"]], dg.recv(s))
        assert (got[s["recv_bytes"]:] == FILL).all()
        assert np.array_equal(host(d_wire), wire)


@pytest.mark.parametrize("base_mis", [0, 2])
@pytest.mark.parametrize("src_mod", range(0, 16, 2))
def test_alignment_matrix(ctx, src_mod, base_mis):
    """Payload start mod 16 (src_mod) x destination mod 16 (all 8) x the payload sizes around every
    chunk boundary; gaps of 18-48 B between destinations keep their sentinel.  base_mis 2: the same
    with the arena itself at 2 mod 16."""
    run(ctx, alignment_case(src_mod, base_mis), base_mis=base_mis)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("layout", ["fixed", "slots", "packed"])
def test_shapes(ctx, count, layout):
    # back to back, then every third image skipped: the others keep their places, the holes their sentinel
    for c in shapes_cases(count, layout):
        run(ctx, c)


@pytest.mark.parametrize("length,count", [(9000, 7), (65536, 5), (65536, 1)])
def test_jumbo(ctx, length, count):
    # fixed stride, then a list with one tiny image among the jumbo ones, in descending order of address
    for c in jumbo_cases(length, count):
        run(ctx, c)


def test_all_skip_empty_and_zero_payload(ctx):
    rng = np.random.default_rng(3)
    arena = rng.integers(0, 256, 100 * 128, dtype=np.uint8)
    offsets, lengths = np.arange(100) * 128, np.full(100, 96)
    check(ctx, arena, offsets, lengths, np.full(100, SKIP, np.uint64), 4096)
    # count == 0: nothing is read, not even null pointers
    d_recv = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    ctx.batch_deliver(None, 0, None, d_recv, 64, offsets=None, lengths=None)
    ctx.batch_deliver(dev(arena), 0, dev(np.zeros(1, np.uint64)), d_recv, 64, stride=128, length=96)
    assert (host(d_recv) == FILL).all()
    # images of 32 bytes have no payload: nothing lands, whatever dst says
    lengths = np.where(np.arange(100) % 2, 32, 96)
    dst, total = back_to_back(lengths, start=0)
    check(ctx, arena, offsets, lengths, dst, total)
    check(ctx, arena, offsets[:1], [32], [0], 64)
    check(ctx, arena, offsets[:3], [32, 32, 32], [0, 8, 16], 64, fixed=(128, 32))


def test_scattered_destinations(ctx):
    """Destinations in shuffled order with gaps of every even size; the gaps keep their sentinel."""
    run(ctx, scattered_case())


def test_guard_rails(ctx):
    """A range that ends exactly at recv_bytes is delivered; one that ends 2 B past it, an odd dst and
    a dst far outside are skipped whole; the bytes after recv_bytes and the neighbours are intact."""
    first, odd, zero = guard_rails_cases()
    got = run(ctx, first)
    recv_bytes, arena = first.recv_bytes, first.arena
    assert np.array_equal(got[recv_bytes - 100:recv_bytes], arena[4 * 256 + 32:4 * 256 + 132])
    assert (got[recv_bytes:] == FILL).all() and (got[200:300] == FILL).all()
    # recv_bytes itself odd or tiny
    run(ctx, odd)
    run(ctx, zero)


def test_past_4gib(ctx):
    """An arena and a receive buffer a little over 4 GiB: images and destinations beyond 2^32 (and one
    pair near the start, so one group of images spans more than a buffer resource can); only the
    regions around the destinations are checked."""
    big = (1 << 32) + (1 << 20)
    d_arena = torch.empty(big, dtype=torch.uint8, device="cuda")
    d_recv = torch.empty(big, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(31)
    offsets = np.asarray([(1 << 32) + 4098, 64, (1 << 32) - 700, (1 << 31) + 6, (1 << 32) + 300000, 8192], np.uint64)
    lengths = np.asarray([1492, 608, 1492, 96, 9000, 34], np.uint32)
    dst = np.asarray([(1 << 32) + 1000, (1 << 32) - 300, 10, (1 << 32) + 70006, (1 << 31) + 2, (1 << 32) + 9998], np.uint64)
    images = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in lengths]
    for o, img in zip(offsets.tolist(), images):
        d_arena[o:o + img.size] = dev(img)
    for d, n in zip(dst.tolist(), lengths.tolist()):
        d_recv[max(d - 64, 0):d + n - 32 + 64] = FILL
    ctx.batch_deliver(d_arena, len(dst), dev(dst), d_recv, big, offsets=dev(offsets), lengths=dev(lengths))
    torch.cuda.synchronize()
    for d, n, img in zip(dst.tolist(), lengths.tolist(), images):
        lo = max(d - 64, 0)
        got = d_recv[lo:d + n - 32 + 64].cpu().numpy()
        want = np.full(got.size, FILL, np.uint8)
        want[d - lo:d - lo + n - 32] = img[32:]
        assert np.array_equal(got, want), d
    # a range ending exactly at the buffer's end, past 4 GiB, and one 2 B further
    d_recv[big - 256:] = FILL
    ends = np.asarray([big - 64, big - 200 + 2], np.uint64)
    ctx.batch_deliver(d_arena, 2, dev(ends), d_recv, big, offsets=dev(offsets[3:5]), lengths=dev(np.asarray([96, 232], np.uint32)))
    got = d_recv[big - 256:].cpu().numpy()
    want = np.full(256, FILL, np.uint8)
    want[256 - 64:] = images[3][32:]
    assert np.array_equal(got, want)


def test_round_trip_segment_receive_plan_deliver(ctx):
    """send stream -> batch_segment -> arrivals (some damaged, re-sent later, go-back-N) ->
    batch_receive -> plan_deliver -> batch_deliver == the send stream."""
    import tcpck
    rng = np.random.default_rng(41)
    seg, stride = 1460, 1504
    stream = rng.integers(0, 256, seg * 4000 + 2, dtype=np.uint8)
    nseg = 4001
    tmpl = np.zeros(32, np.uint8)
    tmpl[0:8] = (127, 0, 0, 1, 127, 0, 0, 1)
    tmpl[9] = 6
    tmpl[20:24] = (0, 0, 0x13, 0x88)  # ack 5000, network order
    tmpl[25] = 0x08                   # the reference's ACK bit
    tmpl[26:28] = (4, 0)
    seq0 = 0xFFFFFFFF - 100000        # wraps inside the stream
    n_dmg = 40
    d_arena = torch.zeros((nseg + n_dmg) * stride, dtype=torch.uint8, device="cuda")
    assert ctx.batch_segment(dev(stream), stream.size, seg, tmpl, seq0, d_arena, stride) == nseg
    # damaged copies after the images; the arrival order names slots of the arena
    victims = np.sort(rng.choice(nseg - 3, n_dmg, replace=False))
    arena = host(d_arena).copy()
    for j, v in enumerate(victims):
        slot = (nseg + j) * stride
        arena[slot:slot + stride] = arena[v * stride:(v + 1) * stride]
        arena[slot + int(rng.integers(0, 32 + seg))] ^= 1 << int(rng.integers(0, 8))
    arrivals, hit = [], dict(zip(victims.tolist(), range(n_dmg)))
    for k in range(nseg):
        if k in hit:  # the damaged copy, two that run ahead, then k again
            arrivals += [nseg + hit[k], k + 1, k + 2]
        arrivals.append(k)
    slots = np.asarray(arrivals)
    n = slots.size
    offsets = (slots * stride).astype(np.uint64)
    lengths = np.where(slots % nseg == nseg - 1, 32 + 2, 32 + seg).astype(np.uint32)
    lengths[slots >= nseg] = 32 + seg
    d_arena = dev(arena)
    d_off, d_len = dev(offsets), dev(lengths)
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    hdr = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    ctx.batch_receive(d_arena, n, ok, hdr, offsets=d_off, lengths=d_len)
    h_hdr, h_ok = host(hdr), host(ok)
    assert int((h_ok == 0).sum()) == n_dmg
    want = dict(rcv_nxt=seq0, snd_nxt=5000, snd_una=4000, rcv_wnd=0, delivered=0)
    w_dst, w_verdict, _, w_used = plan_np(h_hdr, h_ok, lengths, want, stream.size)
    st = tcpck.RcvState(seq0, 5000, 4000, 0, 0, 0)
    dst, verdict, ack, consumed = tcpck.plan_deliver(h_hdr, h_ok, st, stream.size, lengths=lengths)
    assert consumed == w_used == n and st.delivered == want["delivered"] == stream.size
    assert np.array_equal(dst, w_dst) and np.array_equal(verdict, w_verdict)
    assert st.rcv_nxt == (seq0 + stream.size) & 0xFFFFFFFF and st.snd_una == 5000
    d_recv = torch.full((stream.size + 30,), FILL, dtype=torch.uint8, device="cuda")
    ctx.batch_deliver(d_arena, n, dev(dst), d_recv, stream.size, offsets=d_off, lengths=d_len)
    got = host(d_recv)
    assert np.array_equal(got[:st.delivered], stream) and (got[st.delivered:] == FILL).all()


def test_streams(ctx):
    """A non-null stream; two calls on two streams into disjoint halves of one buffer."""
    rng = np.random.default_rng(53)
    n = 600
    lengths = np.asarray((96, 608, 1492))[rng.integers(0, 3, n)]
    offsets = np.arange(n) * 2048
    arena = rng.integers(0, 256, n * 2048, dtype=np.uint8)
    dst, total = back_to_back(lengths, start=6)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    check(ctx, arena, offsets, lengths, dst, total, stream=s1)
    d_arena, d_off, d_len, d_dst = dev(arena), dev(offsets.astype(np.uint64)), dev(lengths.astype(np.uint32)), dev(dst)
    d_recv = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h = n // 2
    ctx.batch_deliver(d_arena, h, d_dst, d_recv, total, offsets=d_off, lengths=d_len, stream=s1)
    ctx.batch_deliver(d_arena, n - h, d_dst[h:], d_recv, total, offsets=d_off[h:], lengths=d_len[h:], stream=s2)
    s1.synchronize()
    s2.synchronize()
    want = np.full(total + 16, FILL, np.uint8)
    deliver_np(arena, offsets, lengths, dst, want[:total])
    assert np.array_equal(host(d_recv), want)
