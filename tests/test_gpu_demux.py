"""GPU tests of the receive demultiplexer: tcpck_batch_demux against the Python
restatement of SocketManager::ReceivePacket's lookup (tests/demux_np.py,
socket-manager.h:187-196) and against the table's own host mirror
(tcpck_conn_table_find), commit's ordering on a stream, the bounds of what the
kernel writes, and the whole ring path receive -> demux -> plan -> deliver on
the reference's two golden sequences interleaved in one ring."""
import numpy as np
import pytest

from deliver_np import SKIP, DeliverGolden
from demux_np import NONE, PORT_1, RST, STATE_KEYS, check_golden_ring, demux_np, golden_ring, header_keys, set_port

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5A5A5A5
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099)
# (entries, max_conns, seed): every table is filled to exactly max_conns, the load at which
# probe runs are longest.  The seeds are chosen so that the key sets of 31, 32, 1000 and 4096
# entries each hold a run that passes the end of the slot array (a host-only table tells:
# test_key_sets_reach_collisions_and_the_wrap_around keeps that from being lost).
TABLES = ((1, 1, 1), (2, 2, 2), (31, 31, 9), (32, 32, 25), (33, 33, 5), (1000, 1000, 2), (4096, 4096, 26))
F_ACK, F_SYN = 0x08, 0x40


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


def ids(n):
    """A device array for n connection ids (u32, held as int32), every entry the sentinel."""
    return dev(np.full(n, SENTINEL, np.uint32).view(np.int32))


def host_ids(t):
    return host(t).view(np.uint32)


def key_set(entries, seed):
    """{key: id}: clustered keys -- consecutive peer ports on one address, consecutive addresses
    on one port, both starting where the seed says -- and up to three listeners; ids are
    arbitrary u32 (not NONE)."""
    rng = np.random.default_rng(seed)
    keys = [(80 + i, 0, 0) for i in range(min(3, entries // 8))]
    port0, addr0 = int(rng.integers(1024, 30000)), 0xC0A80000 + int(rng.integers(0, 1 << 16))
    i = 0
    while len(keys) < entries:
        keys.append((80, 0x0A000001, port0 + i // 2) if i % 2 == 0 else (443, addr0 + i // 2, 50000))
        i += 1
    ids = rng.integers(0, NONE, len(keys), dtype=np.uint64)
    return {k: int(v) for k, v in zip(keys, ids)}


def headers(rng, keys, flag_choices):
    """One random 32-B host-order header per key (host_port, peer_ip, peer_port): every byte
    random -- the destination address at bytes 4-7 included, which the lookup ignores -- but the
    key fields and the SYN / ACK bits, drawn from flag_choices."""
    n = len(keys)
    hdr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k = np.asarray(keys, np.uint64).reshape(n, 3)
    hdr[:, 0:4] = k[:, 1].astype("<u4").view(np.uint8).reshape(n, 4)
    hdr[:, 12:14] = k[:, 2].astype("<u2").view(np.uint8).reshape(n, 2)
    hdr[:, 14:16] = k[:, 0].astype("<u2").view(np.uint8).reshape(n, 2)
    flags = np.asarray(flag_choices, np.uint8)[rng.integers(0, len(flag_choices), n)]
    hdr[:, 25] = (hdr[:, 25] & ~np.uint8(F_ACK | F_SYN)) | flags
    return hdr.reshape(-1)


def traffic(rng, table, count, kind):
    full = [k for k in table if k[1:] != (0, 0)] or list(table)
    listeners = [k for k in table if k[1:] == (0, 0)]
    near = [(hp, ip, pp + 1) for hp, ip, pp in full] + [(hp + 1000, ip, pp) for hp, ip, pp in full] + \
           [(hp, ip ^ (1 << 31), pp) for hp, ip, pp in full] + [(pp, ip, hp) for hp, ip, pp in full]
    misses = [k for k in near if k not in table]
    pick = lambda pool: [pool[i] for i in rng.integers(0, len(pool), count)]
    if kind == "hits":
        hdr = headers(rng, pick(full), (F_ACK, 0, F_ACK | F_SYN))
        if listeners:  # a third of the images: SYNs from anywhere to a listening port
            syn = headers(rng, [(l[0], int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 16))) for l in pick(listeners)],
                          (F_SYN,)).reshape(-1, 32)
            rows = hdr.reshape(-1, 32)
            rows[::3] = syn[::3]
        return hdr
    if kind == "misses":
        return headers(rng, pick(misses), (F_ACK, 0, F_ACK | F_SYN))
    return headers(rng, pick(full + listeners + misses), (F_ACK, 0, F_ACK | F_SYN, F_SYN))


def find_all(table_obj, hdr):
    """tcpck_conn_table_find per image, under the listener rule."""
    host_port, peer_ip, peer_port, flags = header_keys(hdr)
    out = np.empty(host_port.size, np.uint32)
    for k in range(out.size):
        syn = flags[k] & (F_SYN | F_ACK) == F_SYN
        out[k] = table_obj.find(int(host_port[k]), 0 if syn else int(peer_ip[k]), 0 if syn else int(peer_port[k]))
    return out


def demux(ctx, table_obj, hdr, count=None, stream=None, mis=0):
    """batch_demux on a host header array; returns the ids and checks that the 64 entries after
    them keep their sentinel and that the header array is unchanged.  mis: the header array
    starts that many bytes (a multiple of 4) into its allocation."""
    count = hdr.size // 32 if count is None else count
    d_all = torch.zeros(hdr.size + mis + 16, dtype=torch.uint8, device="cuda")
    d_hdr = d_all[mis:mis + hdr.size]
    d_hdr.copy_(torch.from_numpy(hdr))
    d_conn = ids(count + 64)
    torch.cuda.synchronize()
    ctx.batch_demux(table_obj, d_hdr.data_ptr(), count, d_conn, stream=stream)
    got = host_ids(d_conn)
    assert (got[count:] == SENTINEL).all(), "written past d_conn[count)"
    assert np.array_equal(host(d_hdr), hdr), "d_hdr is read only"
    return got[:count]


@pytest.fixture(scope="module")
def tables(ctx):
    import tcpck
    out = {}
    for entries, max_conns, seed in TABLES:
        want = key_set(entries, seed)
        t = tcpck.ConnTable(ctx, max_conns)
        for key, id_ in want.items():
            t.set(*key, id_)
        t.commit()
        out[entries] = (t, want)
    yield out
    for t, _ in out.values():
        t.close()


@pytest.mark.parametrize("entries", [e for e, _, _ in TABLES])
def test_demux_matches_the_lookup_rules(ctx, tables, entries):
    t, want = tables[entries]
    assert t.stats()[:2] == (max(64, 1 << (2 * entries - 1).bit_length()), entries)
    rng = np.random.default_rng(100 + entries)
    seen = set()
    for count in COUNTS:
        for kind in ("hits", "misses", "mixed"):
            hdr = traffic(rng, want, count, kind)
            got = demux(ctx, t, hdr, mis=4 * (count % 4))
            exp = demux_np(hdr, want)
            assert np.array_equal(got, exp), (count, kind, np.flatnonzero(got != exp)[:8])
            if count <= 1000:
                assert np.array_equal(got, find_all(t, hdr)), (count, kind)
            if kind == "hits":
                assert (exp != NONE).all()
            if kind == "misses":
                assert (exp == NONE).all()
            seen.add((kind, bool((exp == NONE).any()), bool((exp != NONE).any())))
    assert ("mixed", True, True) in seen


def test_key_sets_reach_collisions_and_the_wrap_around(tables):
    """The coverage the matrix above relies on: over its seeded key sets some lookups inspect
    three slots or more, and some probe runs pass the end of the slot array."""
    stats = {e: t.stats() for e, (t, _) in tables.items()}
    assert max(s[2] for s in stats.values()) >= 3, stats
    assert max(s[3] for s in stats.values()) >= 1, stats


def test_every_key_of_a_full_table_is_found(ctx, tables):
    """The table filled to exactly max_conns: one image per entry, each entry's own id back."""
    t, want = tables[4096]
    keys = list(want)
    rng = np.random.default_rng(3)
    hdr = headers(rng, [k if k[1:] != (0, 0) else (k[0], 7, 7) for k in keys], (F_ACK,))
    rows = hdr.reshape(-1, 32)
    for i, k in enumerate(keys):
        if k[1:] == (0, 0):
            rows[i, 25] = (rows[i, 25] & ~np.uint8(F_ACK)) | F_SYN
    got = demux(ctx, t, hdr)
    assert got.tolist() == [want[k] for k in keys]


def test_key_rules(ctx):
    import tcpck
    A = 0x0A000001
    want = {(80, 0, 0): 1, (80, A, 4000): 2, (81, A, 4000): 3, (80, A + 1, 4000): 4, (80, A, 4001): 5}
    cases = [  # (host_port, peer_ip, peer_port, flags, expected)
        (80, A, 4000, F_SYN, 1),             # SYN without ACK: the listener, whatever the peer
        (80, 0x7F000001, 9, F_SYN, 1),
        (80, A, 4000, F_SYN | F_ACK, 2),     # SYN+ACK: the full key
        (80, A, 4000, 0, 2),                 # neither flag: the full key
        (80, A, 4000, F_ACK, 2),
        (81, A, 4000, F_ACK, 3),
        (81, A, 4000, F_SYN, NONE),          # no listener on 81, though the full key is there
        (82, A, 4000, F_SYN, NONE),
        (80, 0, 0, F_ACK, 1),                # peer 0:0 traffic lands on the listener's key
        (80, 0, 0, 0, 1),
        (81, 0, 0, F_ACK, NONE),
        (80, A + 1, 4000, F_ACK, 4),         # consecutive address, consecutive port
        (80, A, 4001, F_ACK, 5),
        (80, A + 2, 4000, F_ACK, NONE),      # equality is exact on every field
        (80, A, 4002, F_ACK, NONE),
        (80, A | 1 << 31, 4000, F_ACK, NONE),
        (4000, A, 80, F_ACK, NONE),          # ports the other way round
        (80 | 1 << 15, A, 4000, F_ACK, NONE),
    ]
    rng = np.random.default_rng(8)
    hdr = headers(rng, [c[:3] for c in cases], (0,))
    rows = hdr.reshape(-1, 32)
    for i, c in enumerate(cases):
        rows[i, 25] |= c[3]
        rows[i, 24] = 0xFF  # (the byte beside the flags is not part of them)
    # the destination address (bytes 4-7) is not looked at: one image with an address of its own
    rows[:, 4:8] = np.frombuffer((0x7F000001).to_bytes(4, "little"), np.uint8)
    rows[4, 4:8] = np.frombuffer((0x08080808).to_bytes(4, "little"), np.uint8)
    with tcpck.ConnTable(ctx, 16) as t:
        for key, id_ in want.items():
            t.set(*key, id_)
        t.commit()
        got = demux(ctx, t, hdr)
        assert got.tolist() == [c[4] for c in cases]
        assert np.array_equal(got, demux_np(hdr, want)) and np.array_equal(got, find_all(t, hdr))
        # an empty committed table: nothing is found
        for key in want:
            t.erase(*key)
        t.commit()
        assert (demux(ctx, t, hdr) == NONE).all() and t.stats()[1:] == (0, 0, 0)


def test_commit_orders_with_the_stream(ctx):
    """demux, then erase + set + commit, then demux, all on one stream and no wait between: the
    first result is the old table's, the second the new one's."""
    import tcpck
    old = key_set(200, 11)
    keys = list(old)
    new = dict(old)
    for k in keys[0:200:4]:
        del new[k]                              # erased
    for k in keys[1:200:4]:
        new[k] = old[k] ^ 0x55                  # overwritten
    added = [(8080, 0x0B000000 + i, 6000) for i in range(50)]
    new.update({k: 777000 + i for i, k in enumerate(added)})
    rng = np.random.default_rng(12)
    pool = keys + added
    hdr = headers(rng, [pool[i] for i in rng.integers(0, len(pool), 1000)], (F_ACK, 0))
    rows = hdr.reshape(-1, 32)
    for i in np.flatnonzero(header_keys(hdr)[1] == 0):  # the listeners' images: SYNs
        rows[i, 25] = F_SYN
    s = torch.cuda.Stream()
    d_hdr = dev(hdr)
    first, second, third = ids(1000), ids(1000), ids(1000)
    with tcpck.ConnTable(ctx, 256) as t:
        for key, id_ in old.items():
            t.set(*key, id_)
        t.commit(s)
        torch.cuda.synchronize()
        ctx.batch_demux(t, d_hdr, 1000, first, stream=s)
        for k in keys[0:200:4]:
            t.erase(*k)
        for k in keys[1:200:4] + added:
            t.set(*k, new[k])
        # the mirror is ahead of the image until the commit
        ctx.batch_demux(t, d_hdr, 1000, second, stream=s)
        assert t.find(*added[0]) == 777000
        t.commit(s)
        ctx.batch_demux(t, d_hdr, 1000, third, stream=s)
        s.synchronize()
        exp_old, exp_new = demux_np(hdr, old), demux_np(hdr, new)
        assert np.array_equal(host_ids(first), exp_old) and np.array_equal(host_ids(second), exp_old)
        assert np.array_equal(host_ids(third), exp_new)
        changed = exp_old != exp_new
        assert ((exp_new == NONE) & changed).sum() > 50 and ((exp_old == NONE) & changed).sum() > 50
        assert ((exp_old != NONE) & (exp_new != NONE) & changed).sum() > 50
        assert t.stats()[1] == len(new)


def test_golden_ring_receive_demux_plan_deliver(ctx):
    """The reference's two arrival sequences interleaved in one ring with images to an unknown
    port among them: batch_receive -> batch_demux -> D2H -> plan_deliver_multi -> ONE
    batch_deliver.  Each connection's window of the shared buffer is the reference's recv_buffer,
    every guard byte keeps its fill, the ring is unchanged."""
    import tcpck
    FILL = 0xA5
    dg = DeliverGolden()
    ring = golden_ring(dg, tcpck.update16)
    s0, s1 = dg.sequences
    # six images to a port nobody listens on (copies of sequence 0's, three of them damaged)
    wire, offsets, lengths, which = ring["wire"], ring["offsets"].tolist(), ring["lengths"].tolist(), ring["which"].tolist()
    donors = [i for i in range(len(s0["offsets"])) if s0["ok"][i] and s0["lengths"][i] > 100][:6]
    assert len(donors) == 6
    slots = (0, 17, 18, 50, 77, len(which) + 5)  # ring positions (the last: at the very end)
    extra = []
    for j, (i, at) in enumerate(zip(donors, slots)):
        img = dg.wire(s0)[s0["offsets"][i]:s0["offsets"][i] + s0["lengths"][i]].copy()
        set_port(img, 0, 14, 15999, tcpck.update16)
        if j % 2:
            img[40 + j] ^= 0x10
        extra.append((wire.size, img.size, j % 2 == 0))
        wire = np.concatenate([wire, img])
        offsets.insert(at, extra[-1][0])
        lengths.insert(at, img.size)
        which.insert(at, 2)
    ring = dict(wire=wire, offsets=np.asarray(offsets, np.uint64), lengths=np.asarray(lengths, np.uint32),
                which=np.asarray(which))
    n = len(which)
    d_wire, d_off, d_len = dev(wire), dev(ring["offsets"]), dev(ring["lengths"])
    d_ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_hdr = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    d_conn = ids(n)
    torch.cuda.synchronize()
    ctx.batch_receive(d_wire, n, d_ok, d_hdr, offsets=d_off, lengths=d_len)
    hdr, ok = host(d_hdr), host(d_ok)
    exp_hdr, exp_ok = dg.host_headers(wire, ring["offsets"], ring["lengths"])
    assert np.array_equal(hdr, exp_hdr) and np.array_equal(ok, exp_ok)
    host_port, peer_ip, peer_port, _ = header_keys(hdr)
    key = lambda c: next((int(host_port[k]), int(peer_ip[k]), int(peer_port[k])) for k in range(n) if which[k] == c)
    assert key(1)[2] == PORT_1 and key(2)[0] == 15999
    guard = 64
    bases = (0, (s0["recv_bytes"] + guard + 1) & ~1)
    total = bases[1] + s1["recv_bytes"]
    with tcpck.ConnTable(ctx, 8) as t:
        t.set(*key(0), 0)
        t.set(*key(1), 1)
        t.commit()
        ctx.batch_demux(t, d_hdr, n, d_conn)
        conn = host_ids(d_conn)
    assert conn.tolist() == [c if c < 2 else NONE for c in which]
    conns = (tcpck.ConnState * 2)(*[
        tcpck.ConnState(tcpck.RcvState(*(s["initial"][k] for k in STATE_KEYS[:4]), 0, 0), b, s["recv_bytes"], 0, 0, 0)
        for s, b in zip(dg.sequences, bases)])
    dst, verdict, ack = tcpck.plan_deliver_multi(hdr, ok, conn, conns, lengths=ring["lengths"])
    check_golden_ring(dg, ring, hdr, ok, conn, dst, verdict, ack, conns)
    unknown = np.flatnonzero(ring["which"] == 2)
    good = np.asarray([e[2] for e in extra])
    assert ok[unknown].tolist() == good.astype(int).tolist()
    assert verdict[unknown].tolist() == np.where(good, RST, 0).tolist() and (dst[unknown] == SKIP).all()
    acks = np.asarray([int.from_bytes(hdr[32 * k + 20:32 * k + 24].tobytes(), "little") for k in unknown])
    assert ack[unknown].tolist() == np.where(good, acks, 0).tolist()
    d_recv = torch.full((total + guard,), FILL, dtype=torch.uint8, device="cuda")
    ctx.batch_deliver(d_wire, n, dev(dst), d_recv, total, offsets=d_off, lengths=d_len)
    got = host(d_recv)
    assert np.array_equal(got[:s0["recv_bytes"]], dg.recv(s0))
    assert np.array_equal(got[bases[1]:total], dg.recv(s1))
    assert (got[s0["recv_bytes"]:bases[1]] == FILL).all() and (got[total:] == FILL).all()
    assert np.array_equal(host(d_wire), wire)


def test_argument_checks(ctx):
    import tcpck
    L = ctx._L
    d_hdr = torch.zeros(32 * 8 + 16, dtype=torch.uint8, device="cuda")
    d_conn = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h, c = d_hdr.data_ptr(), d_conn.data_ptr()
    with tcpck.ConnTable(ctx, 4) as t, tcpck.ConnTable(None, 4) as host_only:
        t.set(80, 0, 0, 1)
        assert L.tcpck_batch_demux(ctx._h, t._h, h, 8, c, None) == tcpck.EINVAL  # never committed
        assert L.tcpck_batch_demux(ctx._h, t._h, h, 0, c, None) == tcpck.EINVAL
        t.commit()
        host_only.commit()
        assert L.tcpck_batch_demux(ctx._h, host_only._h, h, 8, c, None) == tcpck.EINVAL  # a table of no device
        assert L.tcpck_batch_demux(None, t._h, h, 8, c, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(ctx._h, None, h, 8, c, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(ctx._h, t._h, None, 8, c, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(ctx._h, t._h, h, 8, None, None) == tcpck.EINVAL
        for mis in (1, 2, 3):
            assert L.tcpck_batch_demux(ctx._h, t._h, h + mis, 8, c, None) == tcpck.EINVAL
            assert L.tcpck_batch_demux(ctx._h, t._h, h, 8, c + mis, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(ctx._h, t._h, h, 1 << 60, c, None) == tcpck.EINVAL  # 32 * count overflows
        if torch.cuda.device_count() > 1:  # a table of another device
            with tcpck.Context(1) as other:
                assert L.tcpck_batch_demux(other._h, t._h, h, 8, c, None) == tcpck.EINVAL
        assert L.tcpck_batch_demux(ctx._h, t._h, None, 0, None, None) == tcpck.OK   # nothing to do
        assert (host(d_conn) == 7).all()
        assert L.tcpck_batch_demux(ctx._h, t._h, h + 4, 8, c + 4, None) == tcpck.OK  # 4-B alignment is enough
        got = host(d_conn)
        assert (got[1:9].view(np.uint32) == NONE).all() and got[0] == 7 and (got[9:] == 7).all()
