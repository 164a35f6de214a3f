"""CPU tests of the batched resend pass's host side: tcpck_resend_images and the numpy
restatement tests/resend_np.py against what the reference's own helpers and predicate lines do
(tests/golden/resend_golden.*, from tests/golden/gen_resend.cc), against each other on seeded
queues, the cap rule, idempotence, every argument rule, and a queue drained over several passes.
No GPU call here."""
import ctypes

import numpy as np
import pytest

from oracle.ref16 import resend_batch_np
from resend_np import CLOSED, NONE, RULE_REF, RULE_SERIAL, ResendGolden, interleaved_queue, keep_np, make_queue, resend_np

MODES = (0, 1)
RULES = (RULE_REF, RULE_SERIAL)


@pytest.fixture(scope="module")
def rg():
    return ResendGolden()


def both(tcpck, q, rule, mode, cap=None, arena_bytes=None):
    """tcpck_resend_images and resend_np on copies of the same queue, compared whole; -> (arena after,
    keep, out_offsets, out_lengths, out_conn, src, total)."""
    a1 = q["arena"][:arena_bytes].copy()
    a2 = a1.copy()
    kw = dict(stride=q["stride"], offsets=q["offsets"], lengths=q["lengths"], conn=q["conn"])
    got = tcpck.resend_images(a1, q["snd"], count=q["count"], length=q["length"], out_cap=cap, rule=rule, mode=mode, **kw)
    exp = resend_np(a2, q["snd"], count=q["count"], length=q["length"], cap=cap, rule=rule, mode=mode, **kw)
    assert got[5] == exp[5]
    for g, e, name in zip(got[:5], exp[:5], ("keep", "out_offsets", "out_lengths", "out_conn", "src")):
        assert g.dtype == e.dtype and np.array_equal(g, e), name
    assert np.array_equal(a1, a2), np.flatnonzero(a1 != a2)[:8]
    return (a1,) + got


def test_fixture_covers_what_it_should(rg):
    groups = {c["group"] for c in rg.cases}
    assert {"seq-equal", "seq-above-1", "seq-below-1", "seq-far-below", "wrap", "seq-max", "closed", "random"} <= groups
    assert 180 <= len(rg.cases) <= 260 and rg.blob.size < 167792
    assert {c["payload"] for c in rg.cases if c["shape"] == "data"} == {0, 2, 100, 536, 1460}
    assert {c["shape"] for c in rg.cases} == {"data", "syn", "synack", "fin"}
    keep = rg.keep()
    assert 40 < keep.sum() < len(keep) - 40
    by = lambda g: [c for c in rg.cases if c["group"] == g]
    # the consequences the header states: seq == snd_una keeps a SYN / FIN and drops a data image ...
    assert all(c["keep"] == (c["shape"] != "data") for c in by("seq-equal") if c["snd_una"] != 0xFFFFFFFF)
    # ... whose seq + 1 wraps to 0 at 0xFFFFFFFF, below every snd_una
    assert not any(c["keep"] for c in by("seq-equal") if c["snd_una"] == 0xFFFFFFFF)
    assert not any(c["keep"] for c in by("wrap")) and not any(c["keep"] for c in by("closed"))
    assert [c["keep"] for c in by("seq-max") if c["shape"] != "data"].count(1) == 0
    assert any(c["keep"] for c in by("seq-max") if c["shape"] == "data")
    assert any(c["closed"] and c["seq"] > c["snd_una"] for c in rg.cases)
    for c in rg.cases:
        assert c["syn"] == (c["shape"] in ("syn", "synack")) and c["fin"] == (c["shape"] == "fin")


@pytest.mark.parametrize("mode", MODES)
def test_fixture_queue(built_lib, rg, mode):
    """The whole fixture as one mixed queue, connection k = case k's state: the reference's keep
    decisions and, REF mode, its patched headers byte for byte; RFC 1071 expectations from
    tcpck_fill16 on the REF image."""
    import tcpck
    arena, offsets, lengths, conn, snd = rg.queue()
    if mode == 1:  # the reference has no such mode: the queue's checksums refilled in it
        for o, n in zip(offsets.tolist(), lengths.tolist()):
            tcpck.fill16(arena[o:o + n], 1)
    q = dict(arena=arena, offsets=offsets, lengths=lengths, conn=conn, snd=snd, stride=0, length=0, count=len(rg.cases))
    after, keep, out_off, out_len, out_conn, src, total = both(tcpck, q, RULE_REF, mode)
    assert np.array_equal(keep, rg.keep()) and total == int(rg.keep().sum())
    assert np.array_equal(src, np.flatnonzero(rg.keep())) and np.array_equal(out_conn, src)
    assert np.array_equal(out_off, offsets[src]) and np.array_equal(out_len, lengths[src])
    before = rg.queue()[0]
    for k, c in enumerate(rg.cases):
        o, n = c["off"], c["len"]
        if not c["keep"]:
            assert np.array_equal(after[o:o + n], arena[o:o + n]), k  # dropped: untouched
            continue
        want = before[o:o + n].copy()
        want[:32] = rg.after(c)
        if mode == 1:
            tcpck.fill16(want, 1)
        assert np.array_equal(after[o:o + n], want), (k, c["group"])
        assert tcpck.checksum16(after[o:o + n], mode) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("count,n_conns,seed", [(1, 1, 1), (64, 1, 2), (1000, 7, 3), (5000, 4096, 4), (3000, 40, 5)])
def test_seeded_queues(built_lib, count, n_conns, seed, rule, mode):
    import tcpck
    # offset lists: clean, then with short, odd and out-of-arena images and ids naming no state
    q = make_queue(seed, count, n_conns, mode=mode)
    after, keep, *_, total = both(tcpck, q, rule, mode)
    if count >= 1000:
        assert count // 10 < total < count - count // 10
    flawed = make_queue(seed + 100, count, n_conns, flaws=True, bad_ids=True, mode=mode)
    both(tcpck, flawed, rule, mode)
    # fixed stride, the arena cut short so the last images do not fit; and h_conn NULL
    f = make_queue(seed + 200, count, n_conns, fixed=True, stride=96, mode=mode)
    both(tcpck, f, rule, mode)
    _, keep, *_ = both(tcpck, f, rule, mode, arena_bytes=max(0, (count - 2) * 96 + 40))
    assert not keep[-2:].any()
    both(tcpck, dict(f, conn=None), rule, mode)
    both(tcpck, dict(q, conn=None), rule, mode)
    # no states at all: nothing is kept, nothing written
    a, keep, *_, total = both(tcpck, dict(q, snd=q["snd"][:0]), rule, mode)
    assert total == 0 and np.array_equal(a, q["arena"])


def test_rules_differ_where_they_should(built_lib):
    """REF drops a data image at seq == snd_una and everything across a wrap; SERIAL keeps both."""
    import tcpck
    q = make_queue(7, 4, 1, fixed=True, stride=96, mode=0)
    arena = q["arena"]
    for k, (seq, flags, tcplen) in enumerate([(0xFFFFFFF0, 0x08, 64), (5, 0x08, 64), (0xFFFFFF00, 0x08, 64), (0xFFFFFFF0, 0x08, 0)]):
        arena[96 * k + 16:96 * k + 20] = np.frombuffer(seq.to_bytes(4, "big"), np.uint8)
        arena[96 * k + 25] = flags
        arena[96 * k + 10:96 * k + 12] = [tcplen >> 8, tcplen & 0xFF]
        tcpck.fill16(arena[96 * k:96 * k + 64], 0)
    q["snd"][0] = [0xFFFFFFF0, 77, 0, 0]
    assert both(tcpck, q, RULE_REF, 0)[1].tolist() == [0, 0, 0, 0]
    assert both(tcpck, q, RULE_SERIAL, 0)[1].tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_equals_set_ack_on_the_kept_subset(built_lib, mode):
    """The arena after the pass == resend_batch_np (the reference's rewrite + full recompute) on exactly
    the kept images of a fresh copy, each with its connection's rcv_nxt; and every survivor verifies."""
    import tcpck
    q = make_queue(11, 2000, 9, mode=mode)
    after, keep, out_off, out_len, out_conn, src, total = both(tcpck, q, RULE_REF, mode)
    fresh = q["arena"].copy()
    kept = np.flatnonzero(keep_np(fresh, q["snd"], q["offsets"], q["lengths"], q["conn"], RULE_REF))
    assert np.array_equal(kept, src)
    resend_batch_np(fresh, q["offsets"][kept].astype(np.int64), q["lengths"][kept].astype(np.int64),
                    q["snd"][q["conn"][kept], 1], mode)
    assert np.array_equal(after, fresh)
    assert all(tcpck.checksum16(after[o:o + n], mode) == 0 for o, n in zip(out_off[:300].tolist(), out_len[:300].tolist()))
    assert (np.diff(out_off.astype(np.int64)) > 0).all()  # stable: a sorted queue stays sorted


@pytest.mark.parametrize("mode", MODES)
def test_cap_idempotence_and_guards(built_lib, mode):
    """cap = 0, 1, total - 1, total, total + 1: only the first cap entries of each list are written,
    the total is whole, every kept image is patched, nothing past any output is touched; a second pass
    with the same states returns the same lists and changes no byte; each output may be absent."""
    import tcpck
    L = tcpck.lib()
    q = make_queue(21, 700, 5, mode=mode)
    ref_arena = q["arena"].copy()
    full = resend_np(ref_arena, q["snd"], offsets=q["offsets"], lengths=q["lengths"], conn=q["conn"], mode=mode)
    total = full[5]
    assert 100 < total < 600
    G = 8

    def run(arena, cap, absent=()):
        outs = dict(keep=np.full(700 + G, 0xA5, np.uint8), off=np.full(total + G, 0xA5A5A5A5A5A5A5A5, np.uint64),
                    len=np.full(total + G, 0xA5A5A5A5, np.uint32), conn=np.full(total + G, 0xA5A5A5A5, np.uint32),
                    src=np.full(total + G, 0xA5A5A5A5, np.uint32))
        n = ctypes.c_uint64(99)
        p = lambda k: None if k in absent else outs[k].ctypes.data
        rc = L.tcpck_resend_images(mode, 0, arena.ctypes.data, arena.size, 0, 0, q["offsets"].ctypes.data,
                                   q["lengths"].ctypes.data, q["conn"].ctypes.data, q["snd"].ctypes.data, 5, 700,
                                   p("keep"), p("off"), p("len"), p("conn"), p("src"), cap, ctypes.byref(n))
        assert rc == tcpck.OK and n.value == total
        w = min(cap, total)
        for k, exp, fill in (("off", full[1], 0xA5A5A5A5A5A5A5A5), ("len", full[2], 0xA5A5A5A5),
                             ("conn", full[3], 0xA5A5A5A5), ("src", full[4], 0xA5A5A5A5)):
            if k in absent:
                assert (outs[k] == fill).all()
            else:
                assert np.array_equal(outs[k][:w], exp[:w]) and (outs[k][w:] == fill).all(), (k, cap)
        if "keep" in absent:
            assert (outs["keep"] == 0xA5).all()
        else:
            assert np.array_equal(outs["keep"][:700], full[0]) and (outs["keep"][700:] == 0xA5).all()
        assert np.array_equal(arena, ref_arena), cap  # every kept image patched, whatever the cap

    for cap in (0, 1, total - 1, total, total + 1, 700):
        run(q["arena"].copy(), cap)
    for absent in (("keep",), ("off",), ("len",), ("conn",), ("src",), ("keep", "off", "len", "conn", "src")):
        run(q["arena"].copy(), total, absent)
    run(ref_arena.copy(), total)  # the second pass: same lists, no byte changed
    q2 = dict(q, arena=ref_arena)
    assert np.array_equal(both(tcpck, q2, RULE_REF, mode)[0], ref_arena)


def test_guard_rails_for_connection_ids(built_lib):
    """An id of NONE or >= n_conns: dropped, and no state outside [0, n_conns) is read -- the rows
    after the table would keep everything."""
    import tcpck
    q = make_queue(31, 10, 3, fixed=True, stride=96)
    table = np.zeros((6, 4), np.uint32)
    table[:3] = [0, 9, 0, 0]       # snd_una 0: everything with seq > 0 is owed
    table[3:] = [0, 0xEEEEEEEE, 0, 0]
    q["snd"] = table[:3]
    q["conn"] = np.asarray([0, 1, 2, 3, 4, NONE, 0x80000000, 2, NONE - 1, 0], np.uint32)
    q["arena"][16:960:96] = 1  # every seq >= 2^24
    for k in range(10):
        q["arena"][96 * k + 25] = 0x08
        tcpck.fill16(q["arena"][96 * k:96 * k + 64], 0)
    after, keep, *_ , src, total = both(tcpck, q, RULE_REF, 0)
    assert src.tolist() == [0, 1, 2, 7, 9] and total == 5
    assert not (after.reshape(-1)[:960].reshape(10, 96)[:, 20:24] == 0xEE).all(axis=1).any()
    # a closed connection drops its images untouched
    q["snd"] = table[:3].copy()
    q["snd"][2, 2] = CLOSED | 6
    after, keep, *_ = both(tcpck, q, RULE_REF, 0)
    assert keep.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1] and np.array_equal(after[192:288], q["arena"][192:288])


def test_argument_checks_write_nothing(built_lib):
    import tcpck
    L = tcpck.lib()
    q = make_queue(3, 50, 4)
    raw = np.zeros(q["arena"].size + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    arena = raw[at:at + q["arena"].size + 2]
    arena[:q["arena"].size] = q["arena"]
    before = raw.copy()
    snd_raw = np.zeros(4 * 4 + 8, np.uint32)
    s_at = ((-snd_raw.ctypes.data) % 16) // 4
    snd = snd_raw[s_at:s_at + 16 + 2]
    snd[:16] = q["snd"].reshape(-1)
    keep = np.full(51, 0xA5, np.uint8)
    out_off = np.full(52, 7, np.uint64)
    out_len, out_conn, src = (np.full(52, 0xA5A5A5A5, np.uint32) for _ in range(3))
    total = (ctypes.c_uint64 * 2)(77, 77)
    good = dict(mode=0, rule=0, arena=arena.ctypes.data, arena_bytes=q["arena"].size, stride=0, len=0,
                offsets=q["offsets"].ctypes.data, lengths=q["lengths"].ctypes.data, conn=q["conn"].ctypes.data,
                snd=snd.ctypes.data, n_conns=4, count=50, keep=keep.ctypes.data, out_off=out_off.ctypes.data,
                out_len=out_len.ctypes.data, out_conn=out_conn.ctypes.data, src=src.ctypes.data, cap=50,
                total=ctypes.addressof(total))

    def call(**kw):
        a = {**good, **kw}
        a["total"] = ctypes.cast(a["total"], ctypes.POINTER(ctypes.c_uint64)) if a["total"] else None
        return L.tcpck_resend_images(*a.values())

    fixed = dict(offsets=None, lengths=None, stride=96, len=64)
    bad = [dict(mode=2), dict(mode=-1), dict(rule=2), dict(rule=-1), dict(count=(1 << 31) + 1), dict(arena=None),
           dict(snd=None), dict(total=None), dict(lengths=None), dict(offsets=None),
           dict(fixed, stride=95), dict(fixed, len=63, stride=96), dict(fixed, len=30), dict(fixed, stride=62),
           dict(fixed, len=0, stride=0),
           dict(arena=good["arena"] + 1), dict(lengths=good["lengths"] + 2), dict(conn=good["conn"] + 1),
           dict(out_len=good["out_len"] + 2), dict(out_conn=good["out_conn"] + 1), dict(src=good["src"] + 3),
           dict(offsets=good["offsets"] + 4), dict(out_off=good["out_off"] + 4), dict(total=good["total"] + 4),
           dict(snd=good["snd"] + 8), dict(count=0, mode=5), dict(count=0, rule=5), dict(count=0, lengths=None)]
    for kw in bad:
        assert call(**kw) == tcpck.EINVAL, kw
        assert np.array_equal(raw, before) and (keep == 0xA5).all() and (out_off == 7).all(), kw
        assert all((a == 0xA5A5A5A5).all() for a in (out_len, out_conn, src)) and list(total) == [77, 77], kw
    # count == 0: the count comes back 0 and nothing else is needed
    assert call(count=0, arena=None, snd=None, n_conns=0, conn=None, keep=None, out_off=None, out_len=None,
                out_conn=None, src=None) == tcpck.OK
    assert total[0] == 0 and total[1] == 77
    assert call(count=0, total=None) == tcpck.OK
    assert call(count=0, arena=None, **fixed) == tcpck.OK
    # the alignments that are enough
    assert call(arena=good["arena"] + 2, arena_bytes=q["arena"].size - 2, total=good["total"] + 8, src=good["src"] + 4,
                out_off=good["out_off"] + 8, snd=good["snd"] + 16, n_conns=3, count=0) == tcpck.OK


def test_scratch_bytes(built_lib):
    import tcpck
    L = tcpck.lib()
    counts = (0, 1, 16, 17, 1024, 1025, 1 << 20, (1 << 20) + 3, 1 << 31)
    sizes = [tcpck.resend_scratch_bytes(n) for n in counts]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    # a u32 per block of 1024 images and a keep byte per image, each rounded up to 16 B
    assert sizes[:6] == [16, 32, 32, 48, 16 + 1024, 16 + 1040] and sizes[-1] == (1 << 23) + (1 << 31)
    out = ctypes.c_size_t(5)
    assert L.tcpck_resend_scratch_bytes((1 << 31) + 1, ctypes.byref(out)) == tcpck.EINVAL and out.value == 5
    assert L.tcpck_resend_scratch_bytes(8, None) == tcpck.EINVAL


def drain(step, seed, mode, rule=RULE_REF):
    """Three connections' queues made by segment_np, interleaved; snd_una advanced each round by a
    seeded number of segments; the lists ping-ponged through step(arena, offsets, lengths, conn, snd)
    -> (out_offsets, out_lengths, out_conn, total) until the queue is empty.  -> the rounds taken."""
    q = interleaved_queue(seed, mode=mode, wrap=rule == RULE_SERIAL)
    rng = np.random.default_rng(seed)
    arena, offsets, lengths, conn = q["arena"], q["offsets"], q["lengths"], q["conn"]
    acked = [0, 0, 0]
    rounds = 0
    while offsets.size:
        rounds += 1
        assert rounds < 100
        snd = np.zeros((3, 4), np.uint32)
        for c in range(3):
            acked[c] = min(q["nseg"][c], acked[c] + int(rng.integers(0, 4)))
            # the last segment may be short, and REF keeps an image until snd_una passes its seq
            snd[c, 0] = (q["seq0"][c] + acked[c] * q["seg"] + (q["seg"] if acked[c] == q["nseg"][c] else 0)) & 0xFFFFFFFF
            snd[c, 1] = rng.integers(0, 1 << 32)
        offsets, lengths, conn, total = step(arena, offsets, lengths, conn, snd)
        assert total == offsets.size
    return rounds


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("seed", (1, 2))
def test_queue_loop(built_lib, seed, rule, mode):
    """The model and the twin agree every round and take the round count the model alone gives.  Under
    the serial rule connection 0's sequence numbers pass 2^32 on the way."""
    import tcpck
    seen = []

    def model_step(arena, offsets, lengths, conn, snd):
        r = resend_np(arena, snd, offsets=offsets, lengths=lengths, conn=conn, rule=rule, mode=mode)
        seen.append((arena.copy(), r))
        return r[1], r[2], r[3], r[5]

    alone = drain(model_step, seed, mode, rule)
    trace = iter(list(seen))

    def twin_step(arena, offsets, lengths, conn, snd):
        got = tcpck.resend_images(arena, snd, offsets=offsets, lengths=lengths, conn=conn, rule=rule, mode=mode)
        exp_arena, exp = next(trace)
        assert np.array_equal(arena, exp_arena)
        assert all(np.array_equal(g, e) for g, e in zip(got[:5], exp[:5])) and got[5] == exp[5]
        return got[1], got[2], got[3], got[5]

    assert drain(twin_step, seed, mode, rule) == alone > 3
