"""GPU tests of tcpck_batch_deliver's group machinery (tcp-stack_amd/csrc/
tcpck_deliver.hip): several images in one block -- the 64-lane scan over more
than one live lane, the 6-probe search, the ds_bpermute pulls, steps shared by
the chunks of several images -- and several groups in one block (the in-flight
descriptor prefetch, a partial last group).  The launcher puts one image in a
block below 12,288 images and walks a second group only above 6.3 million, so
the small cases here fix the grid through the probe library
(tcpck_probe_set_deliver_grid: the product's kernel, another split of the batch
over the blocks) and assert, through its read-back, that the split they were
written for was the one launched; the last two tests run the product library at
counts where its own rule reaches both regimes.

Every case pre-fills the receive buffer with 0xA5, compares it WHOLE with
tests/deliver_np.py and checks that the arena is unchanged (test_gpu_deliver's
check()); the > 1 GiB cases compare the regions around every destination."""
import numpy as np
import pytest

from deliver_cases import (Case, alignment_case, back_to_back, guard_rails_cases, jumbo_cases, scattered_case,
                           shapes_cases)
from deliver_np import SKIP, deliver_np_fast
from test_gpu_deliver import FILL, dev, host, run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# name -> (run, max_blocks) of tcpck_probe_set_deliver_grid
GRIDS = {"run=64": (64, 0), "max_blocks=1": (0, 1), "max_blocks=2": (0, 2), "run=3": (3, 0), "product": (0, 0)}
FORCED = ("run=64", "max_blocks=1", "max_blocks=2", "run=3")


@pytest.fixture(scope="module")
def probe_ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available()
    c = tcpck.Context(0, probe=True)
    yield c
    c.set_deliver_grid(0, 0)
    c.close()


@pytest.fixture
def pctx(probe_ctx):
    yield probe_ctx
    probe_ctx.set_deliver_grid(0, 0)


def split_of(grid, count):
    """(blocks, per_block, rem) the launcher must report for `count` images under `grid`.  The
    counts here stay below every threshold of the launcher's own rule (one image per block below
    4 x the resident grid, a cap of 64 x the resident grid), whatever the occupancy."""
    run_, cap = GRIDS[grid]
    blocks = -(-count // (run_ or 1))
    if cap:
        blocks = min(blocks, cap)
    return blocks, count // blocks, count % blocks


def run_grid(pctx, grid, case, largest=None, **kw):
    """check() on `case` under `grid`; the launch had the split the grid stands for, and its
    largest block held `largest` images (where the test was written for a number)."""
    pctx.set_deliver_grid(*GRIDS[grid])
    got = run(pctx, case, **kw)
    count = kw.get("count", len(case.dst))
    blocks, per_block, rem = pctx.deliver_split()
    assert (blocks, per_block, rem) == split_of(grid, count), (grid, count)
    if grid == "max_blocks=1":
        assert blocks == 1 and per_block == count
    if largest is not None:
        assert per_block + (rem > 0) == largest, (per_block, rem, largest)
    return got


def test_grid_hook_reads_back_and_resets(pctx):
    c = shapes_cases(257, "slots")[0]
    assert run_grid(pctx, "run=64", c, largest=52) is not None  # 5 blocks: 2 of 52 images, 3 of 51
    assert pctx.deliver_split() == (5, 51, 2)
    run_grid(pctx, "max_blocks=2", c, largest=129)
    run_grid(pctx, "run=3", c, largest=3)
    assert pctx.deliver_split() == (86, 2, 85)  # 85 blocks of 3 images and a short last one
    run_grid(pctx, "product", c, largest=1)
    assert pctx.set_deliver_grid(0, 0) == (257, 1, 0)
    with pytest.raises(Exception):
        pctx.set_deliver_grid(0, (1 << 24) + 1)


# ---- a. the single-image matrices again, several images per block ----------------

@pytest.mark.parametrize("grid", FORCED)
@pytest.mark.parametrize("base_mis", [0, 2])
@pytest.mark.parametrize("src_mod", range(0, 16, 2))
def test_alignment_matrix(pctx, src_mod, base_mis, grid):
    """136 images: 3 groups in one block under max_blocks=1, two blocks of 68 under max_blocks=2 (the
    run boundary inside a 64-aligned stretch), 3 blocks of 46 / 45 under run=64."""
    run_grid(pctx, grid, alignment_case(src_mod, base_mis), base_mis=base_mis,
             largest={"run=64": 46, "max_blocks=1": 136, "max_blocks=2": 68, "run=3": 3}[grid])


@pytest.mark.parametrize("grid", FORCED)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("layout", ["fixed", "slots", "packed"])
def test_shapes(pctx, count, layout, grid):
    for c in shapes_cases(count, layout):
        run_grid(pctx, grid, c)


@pytest.mark.parametrize("grid", FORCED)
def test_scattered_destinations(pctx, grid):
    run_grid(pctx, grid, scattered_case())  # 1500 images: 24 groups in the one block of max_blocks=1


@pytest.mark.parametrize("grid", FORCED)
@pytest.mark.parametrize("length,count", [(9000, 7), (65536, 5), (65536, 1)])
def test_jumbo(pctx, length, count, grid):
    for c in jumbo_cases(length, count):
        run_grid(pctx, grid, c)


@pytest.mark.parametrize("grid", FORCED)
def test_guard_rails(pctx, grid):
    first, odd, zero = guard_rails_cases()
    got = run_grid(pctx, grid, first)
    assert np.array_equal(got[4096 - 100:4096], first.arena[4 * 256 + 32:4 * 256 + 132])
    assert (got[4096:] == FILL).all() and (got[200:300] == FILL).all()
    run_grid(pctx, grid, odd)
    run_grid(pctx, grid, zero)


# ---- b. group edges ----------------------------------------------------------------

def listed(rng, payloads, dst=None, live=None, start=6, gap=True):
    """A Case of images with these payload sizes at ascending, 2-B aligned arena offsets; dst back to
    back from `start` unless given; live[k] False: dst[k] = SKIP (its place keeps the sentinel)."""
    lengths = 32 + np.asarray(payloads, np.int64)
    room = lengths + (2 * rng.integers(0, 12, lengths.size) if gap else 0)
    offsets = np.concatenate([[0], np.cumsum(room)[:-1]])
    arena = rng.integers(0, 256, int(room.sum()) + 16, dtype=np.uint8)
    if dst is None:
        dst, total = back_to_back(lengths, start=start)
    else:
        dst = np.asarray(dst, np.uint64)
        total = int((dst + (lengths - 32).astype(np.uint64)).max())
    dst = dst.copy()
    if live is not None:
        dst[~np.asarray(live, bool)] = SKIP
    return Case(arena, offsets, lengths, dst, total + 10)


LIVE = {"0": [0], "63": [63], "0,63": [0, 63], "alt": list(range(1, 64, 2)), "none": [], "all": list(range(64))}


def live_mask(names):
    m = np.zeros((len(names), 64), bool)
    for g, name in enumerate(names):
        m[g, LIVE[name]] = True
    return m.reshape(-1)


@pytest.mark.parametrize("grid", ["run=64", "max_blocks=1", "max_blocks=2"])
@pytest.mark.parametrize("order", [("none", "0", "63", "0,63", "alt", "none", "all", "none"),
                                   ("63", "none", "none", "0"), ("alt", "0,63", "none"), ("none",)])
def test_live_lanes(pctx, order, grid):
    """Groups whose live images are lane 0, lane 63, both, every other lane or none at all (T == 0:
    no step), the all-skip group first, in the middle and last in its block."""
    rng = np.random.default_rng(len(order))
    n = 64 * len(order)
    c = listed(rng, 2 * rng.integers(1, 120, n), live=live_mask(order))
    run_grid(pctx, grid, c, largest={"run=64": 64, "max_blocks=1": n, "max_blocks=2": (n + 1) // 2}[grid])


def chunks_of(case, lo, hi):
    """The 16-B destination chunks images [lo, hi) of `case` take, as the kernel counts them."""
    d = np.asarray(case.dst[lo:hi], np.uint64)
    p = (np.asarray(case.lengths[lo:hi], np.int64) - 32).astype(np.uint64)
    keep = d != np.uint64(SKIP)
    d, p = d[keep].astype(np.int64), p[keep].astype(np.int64)
    return int((((d + p + 15) >> 4) - (d >> 4)).sum())


def chunk_total_group(total):
    """(payloads, dst offsets within the group's 2048-B stretch, live) of 64 images whose chunks sum to `total`."""
    pay, at, live = np.full(64, 16), 16 * np.arange(64) * 2, np.ones(64, bool)
    if total == 128:
        pay[:] = 32
    elif total == 63:
        live[17] = False
    elif total == 65:
        at[40] += 8  # 16 B at 8 mod 16: two chunks
    elif total == 1:
        live[:] = False
        live[29] = True
        pay[29] = 2
    return pay, at, live


@pytest.mark.parametrize("grid", ["run=64", "max_blocks=1"])
def test_chunk_totals(pctx, grid):
    """Groups whose chunk total is exactly 64, 128, 63, 65 and 1: the last step full, one lane
    short, one lane over; as blocks of their own and as the five groups of one block."""
    rng = np.random.default_rng(5)
    totals = (64, 128, 63, 65, 1)
    parts = [chunk_total_group(t) for t in totals]
    pay = np.concatenate([p[0] for p in parts])
    at = np.concatenate([p[1] + 2048 * g for g, p in enumerate(parts)])
    live = np.concatenate([p[2] for p in parts])
    c = listed(rng, pay, dst=at, live=live)
    for g, t in enumerate(totals):
        assert chunks_of(c, 64 * g, 64 * g + 64) == t
    run_grid(pctx, grid, c, largest=64 if grid == "run=64" else 320)


@pytest.mark.parametrize("payload", [2, 14, 16, 18])
@pytest.mark.parametrize("start", [0, 6])
def test_images_share_a_chunk(pctx, payload, start):
    """64 payloads packed back to back: at 2 B, 8 images write disjoint bytes of one 16-B chunk; at
    14 / 16 / 18 B every chunk boundary falls at another place of its image."""
    rng = np.random.default_rng(payload)
    run_grid(pctx, "run=64", listed(rng, np.full(64, payload), start=start), largest=64)
    run_grid(pctx, "max_blocks=1", listed(rng, np.full(130, payload), start=start), largest=130)


@pytest.mark.parametrize("grid", ["run=64", "max_blocks=1"])
@pytest.mark.parametrize("descending", ["dst", "src"])
def test_opposite_orders(pctx, descending, grid):
    """Destinations strictly descending inside every group while the sources ascend, and the reverse."""
    rng = np.random.default_rng(9)
    n = 150
    c = listed(rng, 2 * rng.integers(1, 200, n))
    dst, _ = back_to_back(c.lengths[::-1], start=4)
    c = c._replace(dst=dst[::-1].copy())  # image 0 last in the stream
    assert (np.diff(c.dst.astype(np.int64)) < 0).all() and (np.diff(c.offsets) > 0).all()
    if descending == "src":
        c = c._replace(offsets=c.offsets[::-1].copy(), lengths=c.lengths[::-1].copy(), dst=c.dst[::-1].copy())
        assert (np.diff(c.dst.astype(np.int64)) > 0).all() and (np.diff(c.offsets) < 0).all()
    run_grid(pctx, grid, c, largest=50 if grid == "run=64" else n)


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_jumbo_among_tiny(pctx, lane):
    """One 64-KiB image at lane 0, 31 or 63 of a group of 2-B payloads: 4097 chunks of one image, then
    (or before) chunks of 63 others in one step."""
    rng = np.random.default_rng(lane)
    pay = np.full(64, 2)
    pay[lane] = 65536 - 32
    run_grid(pctx, "run=64", listed(rng, pay), largest=64)


@pytest.mark.parametrize("layout", ["fixed", "lists"])
@pytest.mark.parametrize("count", [65, 127, 128, 129])
def test_partial_last_group(pctx, count, layout):
    """One block walks 2 or 3 groups, the last of 1, 63, 64 and 1 images: the descriptors of the
    group after are loaded while a group streams, and only `k < ke` keeps that load inside the
    arrays, which are exactly `count` long (torch tensors of that size)."""
    rng = np.random.default_rng(count)
    if layout == "fixed":
        lengths = np.full(count, 96)
        arena = rng.integers(0, 256, 100 * count, dtype=np.uint8)
        dst, total = back_to_back(lengths, start=2)
        c = Case(arena, 100 * np.arange(count), lengths, dst, total + 4, (100, 96))
    else:
        c = listed(rng, 2 * rng.integers(1, 300, count))
    run_grid(pctx, "max_blocks=1", c, largest=count)


@pytest.mark.parametrize("layout", ["fixed", "lists"])
@pytest.mark.parametrize("grid", ["max_blocks=1", "max_blocks=2", "run=64"])
def test_images_after_the_batch_leave_no_trace(pctx, grid, layout):
    """The device arrays go on past `count` with descriptors as good as the batch's own: the last
    group of the last block is partial, and nothing of what follows it is delivered."""
    rng = np.random.default_rng(13)
    count, more = 65 + 64, 320  # (whatever the kernel prefetches past `count` is still inside the arrays)
    if layout == "fixed":
        lengths = np.full(more, 96)
        arena = rng.integers(0, 256, 100 * more, dtype=np.uint8)
        dst, total = back_to_back(lengths, start=2)
        c = Case(arena, 100 * np.arange(more), lengths, dst, total + 4, (100, 96))
    else:
        c = listed(rng, 2 * rng.integers(1, 300, more))
    got = run_grid(pctx, grid, c, count=count)
    assert (got[int(c.dst[count]):] == FILL).all()


# ---- c. guard rails on what the device arrays hold ----------------------------------

def rails_case():
    """208 images in 1024-B slots, back to back in the stream; every fourth breaks one clause of the
    skip rule.  Each keeps the place its payload would have taken, so the valid neighbours abut the
    range a bad one would have hit.  Every offset is an address of the arena."""
    rng = np.random.default_rng(29)
    n = 208
    lengths = (32 + 2 * rng.integers(1, 200, n)).astype(np.uint32)
    offsets = (1024 * np.arange(n) + 2 * rng.integers(0, 200, n)).astype(np.uint64)
    arena = rng.integers(0, 256, 1024 * n, dtype=np.uint8)
    dst, total = back_to_back(lengths, start=8)
    kinds = ("odd_len", "odd_off", 0, 2, 30, 31, 32, (1 << 24) + 2, 0xFFFFFFFE, "odd_dst", "skip")
    bad = np.arange(1, n, 4)
    for j, k in enumerate(bad):
        kind = kinds[j % len(kinds)]
        if kind == "odd_len":
            lengths[k] += 1
        elif kind == "odd_off":
            offsets[k] += 1
        elif kind == "odd_dst":
            dst[k] += 1
        elif kind == "skip":
            dst[k] = SKIP
        else:
            lengths[k] = kind
    return Case(arena, offsets, lengths, dst, total + 8), bad


@pytest.mark.parametrize("grid", ["product", "run=64"])
def test_device_array_guard_rails(pctx, grid):
    """Odd length, odd offset, lengths 0 / 2 / 30 / 31 / 32 / 16 MiB + 2 / 0xFFFFFFFE, odd dst and
    SKIP, one per bad image: each is skipped whole, its would-be range keeps the sentinel and the
    neighbours on both sides land."""
    c, bad = rails_case()
    got = run_grid(pctx, grid, c, largest=1 if grid == "product" else 52)
    good = np.setdiff1d(np.arange(len(c.dst)), bad)
    covered = np.zeros(got.size, bool)
    for k in good.tolist():
        covered[int(c.dst[k]):int(c.dst[k]) + int(c.lengths[k]) - 32] = True
    assert (got[~covered] == FILL).all() and (~covered).sum() > 52 * 2


# ---- d. images up to the 16-MiB limit ------------------------------------------------

BIG = (1 << 24, (1 << 24) + 2, (1 << 20) + 34, 65538)


@pytest.fixture(scope="module")
def big_arena():
    """35 MB: the four large images at 4 mod 16, then 60 images of 34 B."""
    rng = np.random.default_rng(37)
    offsets, at = [], 4
    for ln in BIG:
        offsets.append(at)
        at = (at + ln + 64) // 16 * 16 + 4
    small = at + 40 * np.arange(60)
    arena = rng.integers(0, 256, int(small[-1]) + 64, dtype=np.uint8)
    return arena, np.asarray(offsets), small


@pytest.mark.parametrize("delta", [0, 2])
def test_up_to_16_mib(pctx, big_arena, delta):
    """Lengths 16 MiB (the longest image: delivered), 16 MiB + 2 (skipped, though its range fits),
    1 MiB + 34 and 65,538, the source 0 or 2 mod 4 against the destination: each alone, then the
    four in one group with 2-B payloads between them."""
    arena, big_off, small_off = big_arena
    pctx.set_deliver_grid(*GRIDS["run=64"])
    for off, ln in zip(big_off.tolist(), BIG):
        assert (off + 32 - (16 + delta)) % 4 == delta
        got = run(pctx, Case(arena, [off], [ln], [16 + delta], 16 + delta + ln - 32 + 6))
        assert (got[16 + delta:-6] != FILL).any() == (ln <= 1 << 24), ln
    where = {0: 0, 21: 1, 41: 2, 63: 3}  # lane -> which large image (the gaps keep every source-to-destination delta)
    offsets, lengths = np.empty(64, np.uint64), np.empty(64, np.uint32)
    small = iter(small_off.tolist())
    for lane in range(64):
        offsets[lane] = big_off[where[lane]] if lane in where else next(small)
        lengths[lane] = BIG[where[lane]] if lane in where else 34
    dst, total = back_to_back(lengths, start=8 + delta)
    assert all((int(offsets[l]) + 32 - int(dst[l])) % 4 == delta for l in where)
    got = run_grid(pctx, "run=64", Case(arena, offsets, lengths, dst, total + 2), largest=64)
    skipped = got[int(dst[21]):int(dst[22])]
    assert (skipped == FILL).all() and skipped.size == (1 << 24) + 2 - 32


# ---- e. the extent window -------------------------------------------------------------

GIB = (1 << 30) + (1 << 20)
HALF = 1 << 29
# against the leader in the middle: two or three images on each side of both window edges
SPREAD = (0, -HALF - 2, -HALF, -HALF + 2, HALF - 2, HALF, HALF + 2, 4096, -4096, HALF - 4096, -HALF + 4096)


def sparse_deliver(pctx, src_at, lengths, dst_at, arena_bytes, recv_bytes):
    """Delivers images at src_at (they may overlap: the arena is only read) to dst_at (disjoint) with
    uninitialised buffers of the given sizes: only the image regions are written, only the regions
    around the destinations compared."""
    rng = np.random.default_rng(43)
    d_arena = torch.empty(arena_bytes, dtype=torch.uint8, device="cuda")
    d_recv = torch.empty(recv_bytes, dtype=torch.uint8, device="cuda")
    images = {}
    for s, n in sorted(zip(src_at, lengths)):  # overlapping images: the later write of the shared bytes wins
        d_arena[s:s + n] = dev(rng.integers(0, 256, n, dtype=np.uint8))
    for s, n in zip(src_at, lengths):
        images[s] = d_arena[s:s + n].cpu().numpy()
    for d, n in zip(dst_at, lengths):
        d_recv[max(d - 64, 0):d + n - 32 + 64] = FILL
    torch.cuda.synchronize()
    pctx.set_deliver_grid(*GRIDS["run=64"])
    pctx.batch_deliver(d_arena, len(dst_at), dev(np.asarray(dst_at, np.uint64)), d_recv, recv_bytes,
                       offsets=dev(np.asarray(src_at, np.uint64)), lengths=dev(np.asarray(lengths, np.uint32)))
    torch.cuda.synchronize()
    assert pctx.deliver_split() == (1, len(dst_at), 0)
    # expected: the sentinel around every destination, then every payload (ranges 2 B apart share a region)
    for d, n in zip(dst_at, lengths):
        lo, hi = max(d - 64, 0), min(d + n - 32 + 64, recv_bytes)
        want = np.full(hi - lo, FILL, np.uint8)
        for d2, n2, s2 in zip(dst_at, lengths, src_at):
            a, b = max(d2, lo), min(d2 + n2 - 32, hi)
            if a < b:
                want[a - lo:b - lo] = images[s2][32 + a - d2:32 + b - d2]
        assert np.array_equal(d_recv[lo:hi].cpu().numpy(), want), (d, n)
    for s, n in zip(src_at, lengths):
        assert np.array_equal(d_arena[s:s + n].cpu().numpy(), images[s])


@pytest.mark.parametrize("spread", ["src", "dst", "both"])
def test_window_edges(pctx, spread):
    """One group whose leader (lane 0) sits in the middle of a 1 GiB + 1 MiB buffer and whose other
    images sit 2^29 B and 2^29 +- 2 B to either side: a pass takes what lies within 2^29 B below
    and less than 2^29 B above the leader and leaves the rest, several candidates each time."""
    mid = HALF + (1 << 19)
    n = len(SPREAD)
    far = [mid + s for s in SPREAD]
    wish = [568, 64, 2, 1460, 2, 576, 64, 2, 1460, 64, 600]  # payloads; sources may overlap, destinations not
    near_src = (4 + 1600 * np.arange(n)).tolist()
    src_at = far if spread != "dst" else near_src
    if spread == "src":
        lengths = [32 + w for w in wish]
        dst, total = back_to_back(lengths, start=6)
        dst_at = dst.tolist()
    else:  # (for both: the destinations in the opposite order of the sources)
        dst_at = far if spread == "dst" else far[:1] + far[:0:-1]
        # an image's payload ends where the next destination above it begins: 2 B at the window's edges
        lengths = [32 + min([w] + [d2 - d for d2 in dst_at if d2 > d]) for d, w in zip(dst_at, wish)]
        assert sorted(set(lengths))[0] == 34 and max(lengths) == 32 + 1460
    sparse_deliver(pctx, src_at, lengths, dst_at, GIB if spread != "dst" else 1600 * n + 64,
                   GIB if spread != "src" else total + 64)


def test_widest_extent(pctx):
    """64 images of 1 MiB at 16-MiB strides, the one in the middle first: one pass whose source
    extent is all but 2^30 B."""
    g = torch.Generator(device="cuda").manual_seed(47)
    ln = (1 << 20) + 32
    d_arena = torch.empty(GIB, dtype=torch.uint8, device="cuda")
    order = [32] + [k for k in range(64) if k != 32]
    offsets = np.asarray([k << 24 for k in order], np.uint64)
    for o in offsets.tolist():
        d_arena[o:o + ln] = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=g)
    dst, total = back_to_back(np.full(64, ln), start=14)
    d_recv = torch.full((total + 18,), FILL, dtype=torch.uint8, device="cuda")
    want = d_recv.clone()
    for o, d in zip(offsets.tolist(), dst.tolist()):
        want[d:d + ln - 32] = d_arena[o + 32:o + ln]
    before = [d_arena[o:o + ln].clone() for o in offsets.tolist()]
    torch.cuda.synchronize()
    pctx.set_deliver_grid(*GRIDS["run=64"])
    pctx.batch_deliver(d_arena, 64, dev(dst), d_recv, total, offsets=dev(offsets),
                       lengths=dev(np.full(64, ln, np.uint32)))
    torch.cuda.synchronize()
    assert pctx.deliver_split() == (1, 64, 0)
    assert torch.equal(d_recv, want)
    assert all(torch.equal(d_arena[o:o + ln], b) for o, b in zip(offsets.tolist(), before))


# ---- f. the product library at the product's own grid ----------------------------------

@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    c = tcpck.Context(0)
    yield c
    c.close()


def test_product_grid_full_groups(ctx, pctx):
    """2^19 packed images of 32-110 B, one in seven skipped: the launcher's own rule puts 64 images
    in every block (8192 blocks) for any occupancy up to 8 blocks per CU on 256 CUs."""
    rng = np.random.default_rng(59)
    count = 1 << 19
    lengths = (32 + 2 * rng.integers(0, 40, count)).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lengths, dtype=np.uint64)[:-1]]).astype(np.uint64)
    arena = rng.integers(0, 256, int(lengths.sum()), dtype=np.uint8)
    dst, total = back_to_back(lengths, start=6)
    dst[rng.integers(0, 7, count) == 0] = SKIP
    want = deliver_np_fast(arena, offsets, lengths, dst, np.full(total + 10, FILL, np.uint8))
    d_arena, d_off, d_len, d_dst = dev(arena), dev(offsets), dev(lengths), dev(dst)
    for c in (ctx, pctx):
        d_recv = torch.full((total + 10,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.batch_deliver(d_arena, count, d_dst, d_recv, total + 10, offsets=d_off, lengths=d_len)
        got = host(d_recv)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    assert pctx.set_deliver_grid(0, 0) == (count // 64, 64, 0)  # the same sources, the same rule
    assert np.array_equal(host(d_arena), arena)


def test_product_grid_several_groups_per_block(ctx, pctx):
    """12 Mi images of 34 B at a stride of 34 (2-B payloads 2 B apart): past 64 x 64 x the resident
    grid, so every block of the product's own launch walks more than one group."""
    count = 12 << 20
    g = torch.Generator(device="cuda").manual_seed(61)
    d_arena = torch.randint(0, 256, (34 * count,), dtype=torch.uint8, device="cuda", generator=g)
    before = d_arena.clone()
    d_dst = torch.arange(2, 2 * count + 2, 2, dtype=torch.int64, device="cuda")
    d_recv = torch.full((2 * count + 16,), FILL, dtype=torch.uint8, device="cuda")
    want = d_recv.clone()
    want[2:2 * count + 2] = d_arena.view(-1, 34)[:, 32:].reshape(-1)
    torch.cuda.synchronize()
    ctx.batch_deliver(d_arena, count, d_dst, d_recv, 2 * count + 2, stride=34, length=34)
    torch.cuda.synchronize()
    assert torch.equal(d_recv, want) and torch.equal(d_arena, before)
    d_recv.fill_(FILL)
    torch.cuda.synchronize()
    pctx.batch_deliver(d_arena, count, d_dst, d_recv, 2 * count + 2, stride=34, length=34)
    torch.cuda.synchronize()
    blocks, per_block, rem = pctx.set_deliver_grid(0, 0)
    assert per_block > 64 and blocks * per_block + rem == count, (blocks, per_block, rem)
    assert torch.equal(d_recv, want)
