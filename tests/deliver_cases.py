"""The inputs of the tcpck_batch_deliver tests, as plain numpy (no device): each
builder returns Case tuples that tests/test_gpu_deliver.py runs on the product's
grid, tests/test_gpu_deliver_groups.py runs again under forced grids (several
images per block, several groups per block), and tests/test_deliver_plan.py uses
to pin deliver_np_fast to deliver_np."""
from collections import namedtuple

import numpy as np

from deliver_np import SKIP

# fixed: (stride, length) for the fixed-stride entry, else the offset / length lists go to the device
Case = namedtuple("Case", "arena offsets lengths dst recv_bytes fixed recv_alloc", defaults=(None, None))

PAYLOADS = (2, 4, 14, 16, 18, 30, 32, 34, 62, 64, 66, 126, 130, 1022, 1024, 1026, 1460)


def back_to_back(lengths, start=0):
    p = np.asarray(lengths, np.int64) - 32
    return (start + np.concatenate([[0], np.cumsum(p)[:-1]])).astype(np.uint64), int(start + p.sum())


def alignment_case(src_mod, base_mis):
    """Payload start mod 16 (src_mod, with the arena itself at base_mis mod 16) x destination mod 16
    (all 8) x the payload sizes around every chunk boundary, 136 images in a shuffled order; gaps of
    18-48 B between destinations."""
    rng = np.random.default_rng(100 + src_mod + base_mis)
    offsets, lengths, dst = [], [], []
    at_s, at_d = 0, 0
    for dst_mod in range(0, 16, 2):
        for p in PAYLOADS:
            # the payload (image + 32) at src_mod mod 16 of the allocation
            at_s = (at_s + 15) // 16 * 16 + (src_mod - 32 - base_mis) % 16
            offsets.append(at_s)
            lengths.append(32 + p)
            at_s += 32 + p + 2 * int(rng.integers(0, 9))
            at_d = (at_d + 18 + 15) // 16 * 16 + dst_mod
            dst.append(at_d)
            at_d += p
    arena = rng.integers(0, 256, at_s + 16, dtype=np.uint8)
    order = rng.permutation(len(dst))  # images in any order of destination
    offsets, lengths, dst = (np.asarray(v)[order] for v in (offsets, lengths, dst))
    return Case(arena, offsets, lengths, dst, at_d + 32)


def shapes_cases(count, layout):
    """`count` images fixed-stride, in 2048-B slots or packed, delivered back to back; then the same
    with every third image skipped."""
    rng = np.random.default_rng(count)
    fixed = None
    if layout == "fixed":
        length, stride = 1492, 1500
        lengths = np.full(count, length)
        offsets = np.arange(count) * stride
        fixed = (stride, length)
    elif layout == "slots":  # the C3 mix in 2048-B receive slots
        lengths = np.asarray((96, 608, 1492))[rng.integers(0, 3, count)]
        offsets = np.arange(count) * 2048
    else:
        lengths = 32 + 2 * rng.integers(0, 400, count)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    arena = rng.integers(0, 256, int(offsets[-1] + lengths[-1]), dtype=np.uint8)
    dst, total = back_to_back(lengths, start=2 * count % 16)
    holes = dst.copy()
    holes[::3] = SKIP
    return [Case(arena, offsets, lengths, dst, total + 6, fixed), Case(arena, offsets, lengths, holes, total + 6, fixed)]


def jumbo_cases(length, count):
    """Jumbo images at a fixed stride; then a list in descending order of address with one tiny
    image among the jumbo ones, the images 2-B aligned."""
    rng = np.random.default_rng(length + count)
    stride = length + 16
    arena = rng.integers(0, 256, stride * count, dtype=np.uint8)
    lengths = np.full(count, length)
    dst, total = back_to_back(lengths, start=10)
    first = Case(arena, np.arange(count) * stride, lengths.copy(), dst, total + 2, (stride, length))
    lengths[-1] = 32 + 2
    offsets = (np.arange(count) * stride + 2 * np.arange(count))[::-1]
    lengths = lengths[::-1]
    dst, total = back_to_back(lengths, start=4)
    return [first, Case(arena, offsets, lengths, dst, total)]


def scattered_case():
    """Destinations in shuffled order with gaps of every even size."""
    rng = np.random.default_rng(17)
    n = 1500
    lengths = 32 + 2 * rng.integers(0, 120, n)
    lengths[rng.integers(0, n, 20)] = 1492
    offsets = np.arange(n) * 1536 + 2 * rng.integers(0, 8, n)
    arena = rng.integers(0, 256, n * 1536 + 16, dtype=np.uint8)
    gaps = 2 * rng.integers(0, 40, n)
    order = rng.permutation(n)
    dst = np.empty(n, np.int64)
    at = 0
    for k in order:
        at += int(gaps[k])
        dst[k] = at
        at += int(lengths[k]) - 32
    return Case(arena, offsets, lengths, dst.astype(np.uint64), at + 10)


def guard_rails_cases():
    """A range that ends exactly at recv_bytes, one that ends 2 B past it, an odd dst and a dst far
    outside; then recv_bytes itself odd and zero."""
    rng = np.random.default_rng(23)
    n, recv_bytes = 12, 4096
    lengths = np.full(n, 32 + 100)
    offsets = np.arange(n) * 256
    arena = rng.integers(0, 256, n * 256, dtype=np.uint8)
    dst = np.asarray([0, 100, 201, 300, recv_bytes - 100, recv_bytes - 98, recv_bytes, recv_bytes + 2, 1 << 40,
                      (1 << 64) - 2, 3800, 500], np.uint64)
    return [Case(arena, offsets, lengths, dst, recv_bytes, None, recv_bytes + 256),
            Case(arena, offsets[:3], lengths[:3], [0, 100, 200], 299, None, 512),
            Case(arena, offsets[:3], lengths[:3], [0, 100, 200], 0, None, 512)]


def random_rule_case(n, seed):
    """n images in 2048-B slots of which about a third break one clause of the skip rule each (odd
    length, odd offset, length below 32 / of 32 / above 16 MiB, odd dst, SKIP, a range past
    recv_bytes); the valid ones land back to back."""
    rng = np.random.default_rng(seed)
    lengths = (32 + 2 * rng.integers(1, 700, n)).astype(np.uint32)
    offsets = (np.arange(n) * 2048 + 2 * rng.integers(0, 300, n)).astype(np.uint64)
    arena = rng.integers(0, 256, n * 2048 + 4096, dtype=np.uint8)
    dst, total = back_to_back(lengths, start=4)
    kind = rng.integers(0, 27, n)
    lengths[kind == 0] += 1
    offsets[kind == 1] += 1
    lengths[kind == 2] = rng.choice([0, 2, 30, 31], int((kind == 2).sum()))
    lengths[kind == 3] = 32
    lengths[kind == 4] = rng.choice([(1 << 24) + 2, 0xFFFFFFFE, 1 << 31], int((kind == 4).sum()))
    dst[kind == 5] += 1
    dst[kind == 6] = SKIP
    dst[kind == 7] = total + 2 - (lengths[kind == 7].astype(np.uint64) - 32)  # ends 2 B past recv_bytes
    dst[kind == 8] = np.uint64(SKIP - 1) - 2 * rng.integers(0, 40, int((kind == 8).sum()), dtype=np.uint64)
    return Case(arena, offsets, lengths, dst, total)
