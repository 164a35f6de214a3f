"""GPU tests of the batched resend pass: tcpck_batch_resend compared bit-exactly with its host twin
tcpck_resend_images and with the numpy restatement (tests/resend_np.py), on the reference's own
packets and decisions (tests/golden/resend_golden.*), over the counts at which the launch changes
shape, keep patterns that leave waves and blocks empty, the bounds of everything it writes, its
composition with VERIFY and tcpck_batch_set_ack, and a queue drained over several passes with no
host hop between them."""
import ctypes

import numpy as np
import pytest

from resend_np import (ACK, RULE_REF, RULE_SERIAL, ResendGolden, fill_batch_np, interleaved_queue, make_queue, resend_np)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = (0, 1)
RULES = (RULE_REF, RULE_SERIAL)
GUARD = 64           # guard elements after every output array
FILL = 0xA5
BLOCK = 1024         # images per block of the mark and emit passes (tcpck_reply.h)
SCAN = 1024          # block totals the scan takes per step: above BLOCK * SCAN images it carries
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4099)  # the chunk, wave and block edges
BIG = (1 << 20) + 3  # 1025 blocks: the scan's second step


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


def as_i64(a):
    return np.ascontiguousarray(a, np.uint64).view(np.int64)


OUTS = ("keep", "off", "len", "conn", "src")


class Call:
    """One tcpck_batch_resend: the inputs uploaded (the states in an allocation of exactly 16 * n_conns
    bytes, the arena in one of exactly arena_bytes), every output with GUARD sentinel elements after it.
    check() reads everything back and compares whole arrays with the model and the twin."""

    def __init__(self, ctx, q, rule=RULE_REF, mode=0, cap=None, arena_bytes=None, absent=(), stream=None):
        import tcpck
        n = q["count"]
        self.q, self.rule, self.mode, self.absent = q, rule, mode, absent
        self.cap = n if cap is None else cap
        self.before = q["arena"][:arena_bytes].copy()
        self.n_conns = q["snd"].shape[0]
        self.d_arena = dev(self.before)
        self.d_off = None if q["offsets"] is None else dev(as_i64(q["offsets"]))
        self.d_len = None if q["lengths"] is None else dev(as_i32(q["lengths"]))
        self.d_conn = None if q["conn"] is None else dev(as_i32(q["conn"]))
        self.d_snd = dev(as_i32(q["snd"])) if self.n_conns else None
        full = lambda size, dtype, v: torch.full((size + GUARD,), v, dtype=dtype, device="cuda")
        self.d = dict(keep=full(n, torch.uint8, FILL), off=full(self.cap, torch.int64, -1),
                      len=full(self.cap, torch.int32, -1), conn=full(self.cap, torch.int32, -1),
                      src=full(self.cap, torch.int32, -1))
        self.d_count = torch.full((1 + GUARD,), -1, dtype=torch.int64, device="cuda")
        self.scratch_bytes = tcpck.resend_scratch_bytes(n)
        self.d_scratch = torch.full((self.scratch_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arg = lambda k: None if k in absent else self.d[k]
        ctx.batch_resend(self.d_arena, self.before.size, self.d_snd, self.n_conns, n, self.d_count, self.d_scratch,
                         stride=q["stride"], length=q["length"], offsets=self.d_off, lengths=self.d_len, conn=self.d_conn,
                         keep=arg("keep"), out_offsets=arg("off"), out_lengths=arg("len"), out_conn=arg("conn"),
                         src=arg("src"), out_cap=self.cap, rule=rule, mode=mode, stream=stream)

    def check(self, twin=True):
        import tcpck
        q, n = self.q, self.q["count"]
        torch.cuda.synchronize()
        kw = dict(count=n, stride=q["stride"], length=q["length"], offsets=q["offsets"], lengths=q["lengths"],
                  conn=q["conn"], rule=self.rule, mode=self.mode)
        exp_arena = self.before.copy()
        exp = resend_np(exp_arena, q["snd"], cap=self.cap, **kw)
        if twin:
            twin_arena = self.before.copy()
            got = tcpck.resend_images(twin_arena, q["snd"], out_cap=self.cap, **kw)
            assert got[5] == exp[5] and all(np.array_equal(g, e) for g, e in zip(got[:5], exp[:5]))
            assert np.array_equal(twin_arena, exp_arena)
        total = exp[5]
        w = min(total, self.cap)
        arena = self.d_arena.cpu().numpy()
        assert np.array_equal(arena, exp_arena), np.flatnonzero(arena != exp_arena)[:8]
        count = self.d_count.cpu().numpy()
        assert count[0] == total and (count[1:] == -1).all(), "d_count or the bytes after it"
        keep = self.d["keep"].cpu().numpy()
        if "keep" in self.absent:
            assert (keep == FILL).all()
        else:
            assert np.array_equal(keep[:n], exp[0]) and (keep[n:] == FILL).all(), "d_keep or past it"
        for name, e, view in (("off", exp[1], np.uint64), ("len", exp[2], np.uint32), ("conn", exp[3], np.uint32),
                              ("src", exp[4], np.uint32)):
            a = self.d[name].cpu().numpy()
            if name in self.absent:
                assert (a == -1).all(), name
            else:
                assert np.array_equal(a[:w].view(view), e) and (a[w:] == -1).all(), name + " or past it"
        assert (self.d_scratch.cpu().numpy()[self.scratch_bytes:] == FILL).all(), "written past the scratch"
        # the inputs are only read
        if q["offsets"] is not None:
            assert np.array_equal(self.d_off.cpu().numpy().view(np.uint64), q["offsets"])
            assert np.array_equal(self.d_len.cpu().numpy().view(np.uint32), q["lengths"])
        if q["conn"] is not None:
            assert np.array_equal(self.d_conn.cpu().numpy().view(np.uint32), q["conn"])
        if self.n_conns:
            assert np.array_equal(self.d_snd.cpu().numpy().view(np.uint32), q["snd"])
        return exp[0], total


def with_pattern(q, name, seed=0):
    """Rewrites the queue's sequence numbers so that exactly the images of the pattern are owed under
    either rule (data images, TcpLength 2, seq = snd_una + 1 or snd_una - 5), refilling the checksums."""
    count = q["count"]
    k = np.arange(count)
    rng = np.random.default_rng(seed)
    if name == "none":
        m = np.zeros(count, bool)
    elif name == "all":
        m = np.ones(count, bool)
    elif name == "first":
        m = k == 0
    elif name == "last":
        m = k == count - 1
    elif name == "alternating":
        m = k % 2 == 1
    elif name in ("per64", "per256", "per1024"):
        step = int(name[3:])
        m = k % step == (step // 3)
    elif name in ("gaps64", "gaps256", "gaps1024"):  # silent runs of one chunk / one wave / one block: start, middle, end
        run = int(name[4:])
        m = np.ones(count, bool)
        for at in (0, (count // 2) // run * run, max(0, (count - run) // run * run), max(0, count - run)):
            m[at:at + run] = False
    else:
        m = rng.random(count) < {"p1": 0.01, "p50": 0.5, "p90": 0.9}[name]
    arena, snd = q["arena"], q["snd"].copy()
    snd[:, 2] = 0
    snd[:, 0] = np.where((snd[:, 0] < 16) | (snd[:, 0] > 0xFFFFFFF0), 1000, snd[:, 0])
    offsets = np.arange(count, dtype=np.int64) * q["stride"] if q["offsets"] is None else q["offsets"].astype(np.int64)
    lengths = np.full(count, q["length"], np.int64) if q["lengths"] is None else q["lengths"].astype(np.int64)
    c = np.zeros(count, np.int64) if q["conn"] is None else q["conn"].astype(np.int64)
    seq = (snd[c, 0].astype(np.int64) + np.where(m, 1, -5)).astype(np.uint32)
    arena[offsets[:, None] + np.arange(16, 20)] = seq.astype(">u4").view(np.uint8).reshape(-1, 4)
    arena[offsets + 25] = ACK
    arena[offsets + 10] = 0
    arena[offsets + 11] = 2
    fill_batch_np(arena, offsets, lengths, q.get("mode", 0))
    return dict(q, snd=snd), m


PATTERNS = ("none", "all", "first", "last", "alternating", "per64", "per256", "per1024", "gaps64", "gaps256", "gaps1024",
            "p1", "p50", "p90")


COMBOS = [(rule, mode) for rule in RULES for mode in MODES]


def all_counts(ctx):
    """Every count of COUNTS under both rules and both modes.  Seeded queues (SYN / FIN / data, closed
    connections, sequence numbers around snd_una and the wrap): an offset list with flawed images and
    ids naming no state, and the fixed form; then every image kept and none."""
    for count in COUNTS:
        for rule, mode in COMBOS:
            q = make_queue(count, count, 7, flaws=True, bad_ids=True, mode=mode)
            Call(ctx, q, rule, mode).check()
            f = make_queue(count + 1, count, 7, fixed=True, stride=96, mode=mode)
            Call(ctx, f, rule, mode).check()
        for i, name in enumerate(("all", "none")):
            rule, mode = COMBOS[(count + i) % 4]
            p, m = with_pattern(dict(make_queue(count + 2, count, 7, fixed=True, stride=64, mode=mode), mode=mode), name)
            assert Call(ctx, p, rule, mode).check()[1] == int(m.sum()), (count, name)


def all_patterns(ctx):
    """4099 images (five blocks, the last nearly empty) and 2600: empty chunks, waves and blocks at
    the start, the middle and the end; the modes and rules taken in turn."""
    for i, name in enumerate(PATTERNS):
        for count in (4099, 2600):
            rule, mode = COMBOS[(i + count) % 4]
            q = dict(make_queue(5, count, 7, mode=mode), mode=mode)
            p, m = with_pattern(q, name, 5)
            keep, total = Call(ctx, p, rule, mode).check()
            assert total == int(m.sum()) and np.array_equal(keep, m), (name, count)


def all_scan_second_step(ctx):
    """2^20 + 3 images of 32 bytes each: 1025 blocks, so the scan of the block totals takes a second
    step with a carry, and the last block holds three images.  (The scan does not depend on the rule
    or the mode: one queue, the reference's.)"""
    import tcpck
    mode = 0
    q = make_queue(77, BIG, 4096, fixed=True, stride=32, mode=mode)
    assert BIG > BLOCK * SCAN and q["length"] == 32
    c = Call(ctx, q, RULE_REF, mode)
    keep, total = c.check()
    assert BIG // 4 < total < BIG and c.scratch_bytes == 4 * 1028 + BIG + 13
    assert c.scratch_bytes == tcpck.resend_scratch_bytes(BIG)


def all_layouts_and_connections(ctx):
    for rule, mode in COMBOS:
        layouts_and_connections(ctx, rule, mode)


def layouts_and_connections(ctx, rule, mode):
    count = 3000
    q = make_queue(3, count, 40, mode=mode)
    f = make_queue(4, count, 40, fixed=True, stride=96, mode=mode)
    for base in (q, f):
        Call(ctx, base, rule, mode).check()
        # no ids: every image is connection 0 ...
        Call(ctx, dict(base, conn=None), rule, mode).check()
        # ... which a call without states does not have: nothing kept, nothing written
        keep, total = Call(ctx, dict(base, conn=None, snd=base["snd"][:0]), rule, mode).check()
        assert total == 0
        assert Call(ctx, dict(base, snd=base["snd"][:0]), rule, mode).check()[1] == 0
        # ids NONE and >= n_conns: dropped, the states' allocation is exactly theirs
        bad = make_queue(5, count, 40, fixed=base is f, stride=96, bad_ids=True, mode=mode)
        Call(ctx, bad, rule, mode).check()
        Call(ctx, dict(bad, snd=bad["snd"][:1]), rule, mode).check()
    # the fixed form with the arena cut short: the last images do not fit and are not touched
    keep, _ = Call(ctx, f, rule, mode, arena_bytes=(count - 3) * 96 + 62).check()
    assert not keep[-3:].any()
    assert Call(ctx, f, rule, mode, arena_bytes=62).check()[1] == 0  # not one image fits
    # 4096 and 65536 connections
    for n_conns in (4096, 65536):
        Call(ctx, make_queue(6, count, n_conns, mode=mode), rule, mode).check()


def all_fixture_queue(ctx):
    """The reference's own packets and keep decisions; REF mode: its patched headers byte for byte."""
    rg = ResendGolden()
    for mode in MODES:
        fixture_queue(ctx, rg, mode)


def fixture_queue(ctx, rg, mode):
    import tcpck
    arena, offsets, lengths, conn, snd = rg.queue()
    if mode == 1:
        fill_batch_np(arena, offsets, lengths, 1)
    q = dict(arena=arena, offsets=offsets, lengths=lengths, conn=conn, snd=snd, stride=0, length=0, count=len(rg.cases))
    c = Call(ctx, q, RULE_REF, mode)
    keep, total = c.check()
    assert np.array_equal(keep, rg.keep())
    after = c.d_arena.cpu().numpy()
    if mode == 0:
        for case in rg.cases:
            if case["keep"]:
                assert np.array_equal(after[case["off"]:case["off"] + 32], rg.after(case))
    assert all(tcpck.checksum16(after[cs["off"]:cs["off"] + cs["len"]], mode) == 0 for cs in rg.cases if cs["keep"])


def all_out_cap_and_absent_outputs(ctx):
    for mode in MODES:
        out_cap_and_absent_outputs(ctx, mode)


def out_cap_and_absent_outputs(ctx, mode):
    count = 2500
    q = make_queue(8, count, 7, mode=mode)
    total = resend_np(q["arena"].copy(), q["snd"], offsets=q["offsets"], lengths=q["lengths"], conn=q["conn"], mode=mode)[5]
    assert 500 < total < 2000
    for cap in (0, 1, total - 1, total, total + 1):
        assert Call(ctx, q, RULE_REF, mode, cap=cap).check()[1] == total  # (the whole arena patched, whatever the cap)
    for absent in (("keep",), ("off",), ("len",), ("conn",), ("src",), ("off", "len", "conn", "src"), OUTS):
        Call(ctx, q, RULE_REF, mode, cap=total - 1, absent=absent).check()


def idempotent(ctx):
    """A second pass over the patched arena with the same states: the same lists, no byte changed."""
    q = make_queue(9, 5000, 40)
    c1 = Call(ctx, q, RULE_REF, 0)
    c1.check()
    q2 = dict(q, arena=c1.d_arena.cpu().numpy())
    c2 = Call(ctx, q2, RULE_REF, 0)
    c2.check()
    assert torch.equal(c1.d_arena, c2.d_arena)
    assert all(torch.equal(c1.d[k], c2.d[k]) for k in OUTS) and torch.equal(c1.d_count, c2.d_count)


def count_zero(ctx):
    import tcpck
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L = ctx._L
    none = [None] * 5
    assert L.tcpck_batch_resend(ctx._h, 0, 0, None, 0, 64, 32, None, None, None, None, 0, 0, *none, 0, d_count.data_ptr(),
                                None, None) == tcpck.OK
    torch.cuda.synchronize()
    assert d_count.cpu().tolist() == [0, -1]
    assert L.tcpck_batch_resend(ctx._h, 0, 1, None, 0, 64, 32, None, None, None, None, 0, 0, *none, 0, None, None,
                                None) == tcpck.OK


def all_two_streams_and_repeats(ctx):
    """Two calls on two streams on different queues, nothing waited for in between; the same inputs
    again; a second pass over the patched arena."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = make_queue(1, 70000, 7)
    b = make_queue(2, 50001, 40, fixed=True, stride=64, mode=1)
    c1 = Call(ctx, a, RULE_REF, 0, stream=s1)
    c2 = Call(ctx, b, RULE_SERIAL, 1, stream=s2)
    c1.check()
    c2.check()
    # and the same inputs give the same bytes again
    c3 = Call(ctx, a, RULE_REF, 0, stream=s2)
    c3.check(twin=False)
    assert torch.equal(c1.d_arena, c3.d_arena) and all(torch.equal(c1.d[k], c3.d[k]) for k in OUTS)
    idempotent(ctx)


def all_composition(ctx):
    for mode in MODES:
        composition(ctx, mode)


def composition(ctx, mode):
    """After the pass, tcpck_batch_var(VERIFY) over the output lists with the sorted hint verifies
    every survivor, and the arena equals what tcpck_batch_set_ack makes of a fresh copy on the kept
    subset with each image's ack its connection's rcv_nxt."""
    import tcpck
    count = 6000
    q = make_queue(12, count, 40, mode=mode)
    c = Call(ctx, q, RULE_REF, mode)
    keep, total = c.check()
    ok = torch.zeros(total, dtype=torch.uint8, device="cuda")
    lens = c.d["len"][:total].cpu().numpy().view(np.uint32)
    ctx.batch_var(tcpck.OP_VERIFY, c.d_arena, c.d["off"], c.d["len"], total, ok, mode=mode,
                  total_bytes=int(lens.sum()), min_len=int(lens.min()), max_len=int(lens.max()), sorted=True)
    torch.cuda.synchronize()
    assert bool(ok.all().item())
    kept = np.flatnonzero(keep)
    fresh = dev(q["arena"])
    ctx.batch_set_ack(fresh, kept.size, acks=dev(as_i32(q["snd"][q["conn"][kept], 1])),
                      offsets=dev(as_i64(q["offsets"][kept])), mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(fresh, c.d_arena)


def all_queue_loop_on_the_device(ctx):
    for rule, mode in COMBOS:
        queue_loop_on_the_device(ctx, rule, mode)


def queue_loop_on_the_device(ctx, rule, mode):
    """Three connections' send streams cut by tcpck_batch_segment into one arena, their images
    interleaved in the queue; snd_una advanced each round by a seeded number of segments; the lists
    ping-ponged between two sets of device arrays, d_snd refreshed by the caller, until the queue is
    empty.  Compared with the model after every round; the device takes the model's round count."""
    import tcpck
    seg, stride = 64, 96
    ref = interleaved_queue(3, seg=seg, mode=mode, wrap=rule == RULE_SERIAL)
    rng = np.random.default_rng(3)
    nseg, seq0 = ref["nseg"], ref["seq0"]
    # the same images made on the device: connection c's segments at slots base[c] ..
    base = np.concatenate([[0], np.cumsum(nseg)[:-1]])
    n = int(sum(nseg))
    d_arena = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    offsets, lengths, conn = [], [], []
    for slot in range(n):  # the queue interleaves the connections round robin, as ref does
        c = int(ref["conn"][slot])
        k = sum(1 for s in range(slot) if ref["conn"][s] == c)
        offsets.append((int(base[c]) + k) * stride)
        lengths.append(int(ref["lengths"][slot]))
        conn.append(c)
    for c in range(3):
        at = [s for s in range(n) if ref["conn"][s] == c]
        hdr = ref["arena"][int(ref["offsets"][at[0]]):][:32].copy()
        pay = np.concatenate([ref["arena"][int(ref["offsets"][s]) + 32:int(ref["offsets"][s]) + int(ref["lengths"][s])]
                              for s in at])
        ctx.batch_segment(dev(pay), pay.size, seg, hdr, seq0[c], d_arena[int(base[c]) * stride:], stride, mode=mode)
    torch.cuda.synchronize()
    model_arena = d_arena.cpu().numpy()
    offsets, lengths, conn = np.asarray(offsets, np.uint64), np.asarray(lengths, np.uint32), np.asarray(conn, np.uint32)
    sets = [dict(off=torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"),
                 len=torch.full((n + 1,), -1, dtype=torch.int32, device="cuda"),
                 conn=torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")) for _ in range(2)]
    sets[0]["off"][:n], sets[0]["len"][:n], sets[0]["conn"][:n] = dev(as_i64(offsets)), dev(as_i32(lengths)), dev(as_i32(conn))
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_scratch = torch.empty(tcpck.resend_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    d_snd = torch.zeros(12, dtype=torch.int32, device="cuda")
    acked, rounds, live, cur = [0, 0, 0], 0, n, 0
    while live:
        rounds += 1
        assert rounds < 100
        snd = np.zeros((3, 4), np.uint32)
        for c in range(3):
            acked[c] = min(nseg[c], acked[c] + int(rng.integers(0, 4)))
            snd[c, 0] = (seq0[c] + acked[c] * seg + (seg if acked[c] == nseg[c] else 0)) & 0xFFFFFFFF
            snd[c, 1] = rng.integers(0, 1 << 32)
        d_snd.copy_(dev(as_i32(snd)).reshape(-1))  # the caller's refresh
        a, b = sets[cur], sets[1 - cur]
        ctx.batch_resend(d_arena, n * stride, d_snd, 3, live, d_count, d_scratch, offsets=a["off"], lengths=a["len"],
                         conn=a["conn"], out_offsets=b["off"], out_lengths=b["len"], out_conn=b["conn"], out_cap=n,
                         rule=rule, mode=mode)
        exp = resend_np(model_arena, snd, offsets=offsets, lengths=lengths, conn=conn, rule=rule, mode=mode)
        offsets, lengths, conn = exp[1], exp[2], exp[3]
        total = int(d_count.cpu().item())  # (read only to compare and to end the loop)
        assert total == exp[5] <= live
        assert np.array_equal(b["off"].cpu().numpy()[:total].view(np.uint64), offsets)
        assert np.array_equal(b["len"].cpu().numpy()[:total].view(np.uint32), lengths)
        assert np.array_equal(b["conn"].cpu().numpy()[:total].view(np.uint32), conn)
        assert (b["off"].cpu().numpy()[n:] == -1).all()
        assert np.array_equal(d_arena.cpu().numpy(), model_arena), rounds
        live, cur = total, 1 - cur
    assert rounds > 3


# The cases above are grouped into few test functions: the suite runs again for every later change,
# and what a failing case is shows in its assertion message and traceback.

def test_shapes(ctx):
    """The counts at which the launch changes shape, the keep patterns, the scan's second step."""
    all_counts(ctx)
    all_patterns(ctx)
    all_scan_second_step(ctx)


def test_layouts_outputs_and_arguments(ctx):
    """Both forms, ids and states present and absent, the reference's fixture, out_cap, absent outputs,
    every TCPCK_EINVAL clause and count == 0."""
    all_layouts_and_connections(ctx)
    all_fixture_queue(ctx)
    all_out_cap_and_absent_outputs(ctx)
    all_argument_checks(ctx)


def test_streams_composition_and_loop(ctx):
    """Two streams and repeated calls, VERIFY and set_ack composition, the queue drained on the device."""
    all_two_streams_and_repeats(ctx)
    all_composition(ctx)
    all_queue_loop_on_the_device(ctx)


def all_argument_checks(ctx):
    """Every TCPCK_EINVAL clause: nothing is launched, so no output and no arena byte changes; and count
    == 0, which only clears the count."""
    import tcpck
    count_zero(ctx)
    L = ctx._L
    n = 300
    q = make_queue(6, n, 4)
    d_arena = dev(np.concatenate([q["arena"], np.zeros(64, np.uint8)]))
    d_off, d_len, d_conn = dev(as_i64(q["offsets"])), dev(as_i32(q["lengths"])), dev(as_i32(q["conn"]))
    d_snd = dev(as_i32(np.concatenate([q["snd"], q["snd"]])))
    d_keep = torch.full((n + 2,), FILL, dtype=torch.uint8, device="cuda")
    d_o = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    d_l, d_c, d_s = (torch.full((n + 2,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    d_count = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((tcpck.resend_scratch_bytes(n) + 32,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    good = dict(ctx=ctx._h, mode=0, rule=0, arena=d_arena.data_ptr(), arena_bytes=q["arena"].size, stride=0, len=0,
                offsets=d_off.data_ptr(), lengths=d_len.data_ptr(), conn=d_conn.data_ptr(), snd=d_snd.data_ptr(),
                n_conns=4, count=n, keep=d_keep.data_ptr(), out_off=d_o.data_ptr(), out_len=d_l.data_ptr(),
                out_conn=d_c.data_ptr(), src=d_s.data_ptr(), cap=n, total=d_count.data_ptr(),
                scratch=d_scratch.data_ptr(), stream=None)
    call = lambda *a, **kw: L.tcpck_batch_resend(*{**good, **dict(*a), **kw}.values())
    fixed = dict(offsets=None, lengths=None, stride=96, len=64)
    bad = [dict(ctx=None), dict(mode=2), dict(mode=-1), dict(rule=2), dict(rule=-1), dict(count=(1 << 31) + 1),
           dict(arena=None), dict(snd=None), dict(total=None), dict(scratch=None), dict(lengths=None), dict(offsets=None),
           dict(fixed, stride=95), dict(fixed, len=63), dict(fixed, len=30), dict(fixed, stride=62), dict(fixed, len=0, stride=0),
           dict(arena=good["arena"] + 1), dict(lengths=good["lengths"] + 2), dict(conn=good["conn"] + 1),
           dict(out_len=good["out_len"] + 2), dict(out_conn=good["out_conn"] + 1), dict(src=good["src"] + 2),
           dict(offsets=good["offsets"] + 4), dict(out_off=good["out_off"] + 4), dict(total=good["total"] + 4),
           dict(snd=good["snd"] + 8), dict(scratch=good["scratch"] + 8), dict(count=0, mode=9), dict(count=0, rule=9),
           dict(count=0, total=good["total"] + 2), dict(count=0, lengths=None)]
    for kw in bad:
        assert call(kw) == tcpck.EINVAL, kw
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy()[:q["arena"].size], q["arena"])
    assert (d_keep.cpu().numpy() == FILL).all() and (d_o.cpu().numpy() == -1).all()
    assert all((t.cpu().numpy() == -1).all() for t in (d_l, d_c, d_s))
    assert d_count.cpu().tolist() == [-1, -1, -1] and (d_scratch.cpu().numpy() == FILL).all()
    # the alignments that are enough: 2 B for the arena, 4 B for the u32 arrays, 8 B for the u64 arrays and the
    # count, 16 B for the states and the scratch
    m = n - 1
    sub = dict(q, arena=q["arena"].copy(), offsets=q["offsets"][1:], lengths=q["lengths"][1:], conn=q["conn"][1:],
               snd=np.concatenate([q["snd"], q["snd"]])[1:5], count=m)
    assert call(offsets=good["offsets"] + 8, lengths=good["lengths"] + 4, conn=good["conn"] + 4, snd=good["snd"] + 16,
                keep=good["keep"] + 1, out_off=good["out_off"] + 8, out_len=good["out_len"] + 4,
                out_conn=good["out_conn"] + 4, src=good["src"] + 4, total=good["total"] + 8,
                scratch=good["scratch"] + 16, count=m, cap=m) == tcpck.OK
    torch.cuda.synchronize()
    exp = resend_np(sub["arena"], sub["snd"], offsets=sub["offsets"], lengths=sub["lengths"], conn=sub["conn"])
    total = exp[5]
    assert d_count.cpu().tolist() == [-1, total, -1]
    assert np.array_equal(d_arena.cpu().numpy()[:q["arena"].size], sub["arena"])
    keep = d_keep.cpu().numpy()
    assert keep[0] == FILL and np.array_equal(keep[1:1 + m], exp[0]) and keep[1 + m] == FILL
    o = d_o.cpu().numpy()
    assert o[0] == -1 and np.array_equal(o[1:1 + total].view(np.uint64), exp[1]) and (o[1 + total:] == -1).all()
    for t, e in ((d_l, exp[2]), (d_c, exp[3]), (d_s, exp[4])):
        a = t.cpu().numpy()
        assert a[0] == -1 and np.array_equal(a[1:1 + total].view(np.uint32), e) and (a[1 + total:] == -1).all()
    # an odd-halfword arena base: 2-B alignment is enough (the fixed form, images at 2 + 96 k)
    f = make_queue(7, 50, 4, fixed=True, stride=96)
    d_a2 = dev(np.concatenate([np.zeros(2, np.uint8), f["arena"]]))
    d_cn = dev(as_i32(f["conn"]))
    d_sn = dev(as_i32(f["snd"]))
    torch.cuda.synchronize()
    assert call(fixed, arena=d_a2.data_ptr() + 2, arena_bytes=f["arena"].size, conn=d_cn.data_ptr(), snd=d_sn.data_ptr(),
                count=50, keep=None, out_off=None, out_len=None, out_conn=None, src=None, total=good["total"]) == tcpck.OK
    torch.cuda.synchronize()
    e2 = f["arena"].copy()
    t2 = resend_np(e2, f["snd"], count=50, stride=96, length=64, conn=f["conn"])[5]
    assert d_count.cpu().tolist()[0] == t2 and np.array_equal(d_a2.cpu().numpy()[2:], e2)
    out = ctypes.c_size_t()
    assert L.tcpck_resend_scratch_bytes(n, ctypes.byref(out)) == tcpck.OK and out.value == 16 + 304
