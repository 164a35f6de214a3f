"""GPU parity of zero-copy segmentation (tcpck_batch_segment_headers, tcpck_segment_hdr.hip): the
headers, payload offsets, lengths and checksums of a send ring of many connections, bit-exact
against oracle.ref16.segment_np applied per cut, against the host twin (tcpck_segment_headers) and
against the reference's own send path (segment_golden); guard bytes after every output array."""
import numpy as np
import pytest

from segment_headers_np import make_cuts, ring_np
from test_segment_headers import check_golden_rows, golden_ring

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 256


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available()
    c = tcpck.Context(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run(ctx, payload, cuts, tmpl, seg, n_seg, mode=0):
    """The device call on a planned (or damaged) table -> (hdr, pay_off, pay_len, checksums)."""
    outs = [torch.full((w * n_seg + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for w in (32, 8, 4, 2)]
    d_pay, d_cuts, d_tmpl = dev(payload), dev(cuts), dev(tmpl)
    ctx.batch_segment_headers(d_pay, payload.size, seg, d_cuts, cuts.size, d_tmpl, tmpl.shape[0], n_seg, *outs, mode=mode)
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, w in zip(host, (32, 8, 4, 2)):
        assert (h[w * n_seg:] == 0xA5).all(), f"wrote past the end of the {w}-B output"
    return (host[0][:32 * n_seg].reshape(n_seg, 32), host[1][:8 * n_seg].view(np.uint64),
            host[2][:4 * n_seg].view(np.uint32), host[3][:2 * n_seg].view(np.uint16))


def check(ctx, payload, cuts, tmpl, seg, n_seg, mode, skip=(), planned=None, what=""):
    import tcpck
    got = run(ctx, payload, cuts, tmpl, seg, n_seg, mode)
    twin = tcpck.segment_headers(payload, seg, cuts, tmpl, n_seg, mode)
    want = ring_np(payload, cuts if planned is None else planned, tmpl, seg, n_seg, mode, skip)
    for name, g, t, w in zip(("hdr", "pay_off", "pay_len", "checksum"), got, twin, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: device {name} against segment_np")
        np.testing.assert_array_equal(g, t, err_msg=f"{what}: device {name} against the host twin")
    return got


def random_ring(seed):
    """3000 cuts of 0-3 MSS segments, the last one possibly short."""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, 3 * 730 + 1, 3000) * 2]


CASES = {  # seg, cut sizes, offset residues mod 16
    "seg16": (16, [2, 14, 16, 18, 16 * 70 + 6, 18, 16, 14, 2], (0, 4, 8, 12)),
    "seg1024": (1024, [1024 * 300, 1022], (0,)),
    "mss": (1460, [1460, 1462, 2, 0, 1460 * 3, 1460 * 130 + 2], (0,)),
    "mss_many": (1460, random_ring(3), (0,)),
    "jumbo9000": (9000, [9000 * 5 + 14], (0,)),
    "jumbo65532": (65532, [65532 * 2 + 4, 65530], (0,)),
}


def test_planned_rings_against_oracle_twin_and_golden(ctx, segment_golden):
    """Every row of CASES in both modes, then the fixture streams as one ring against the reference's
    own bytes (one test: the suite's count of GPU tests is kept small)."""
    import tcpck
    for name, (seg, sizes, residues) in CASES.items():
        for mode in (0, 1):
            rng = np.random.default_rng(len(sizes) + seg + mode)
            tmpl = rng.integers(0, 256, (7, 32), dtype=np.uint8)
            cuts, size = make_cuts(sizes, rng.integers(0, 1 << 32, len(sizes)), rng.integers(0, 7, len(sizes)), residues)
            cuts["seq0"][0] = 0xFFFFFFF0  # the sequence number wraps in the first cut's second segment, where it has one
            payload = rng.integers(0, 256, size, dtype=np.uint8)
            n_seg = tcpck.plan_cuts(cuts, seg, size, 7)
            check(ctx, payload, cuts, tmpl, seg, n_seg, mode, what=f"{name}, mode {mode}")
    for seg in (16, 1460, 9000):
        payload, cuts, tmpl, n_seg = golden_ring(segment_golden, seg)
        hdr, _, _, cs = check(ctx, payload, cuts, tmpl, seg, n_seg, 0, what=f"golden ring at {seg}")
        check_golden_rows(segment_golden, segment_golden.cases, cuts, seg, hdr, cs)


def test_damaged_table_zeroes_only_the_damaged_cuts(ctx):
    """A `first` out of order, an offset past the arena and a template out of range, each in one cut
    of a planned table: those cuts' segments come back zero, every other segment exact."""
    import tcpck
    rng = np.random.default_rng(17)
    sizes = [int(x) for x in rng.integers(1, 3 * 730 + 1, 40) * 2]
    tmpl = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    planned, size = make_cuts(sizes, rng.integers(0, 1 << 32, 40), rng.integers(0, 3, 40))
    payload = rng.integers(0, 256, size, dtype=np.uint8)
    n_seg = tcpck.plan_cuts(planned, 1460, size, 3)
    cuts = planned.copy()
    cuts[7]["first"] = cuts[5]["first"]
    cuts[20]["offset"] = (size + 3) // 4 * 4
    cuts[30]["tmpl"] = 3
    got = check(ctx, payload, cuts, tmpl, 1460, n_seg, 0, skip=(7, 20, 30), planned=planned)
    f, n = int(planned[7]["first"]), -(-sizes[7] // 1460)
    assert not got[0][f:f + n].any() and not got[2][f:f + n].any()


def test_argument_errors(ctx):
    import tcpck
    cuts, size = make_cuts([1460 * 2], [5], [0])
    n_seg = tcpck.plan_cuts(cuts, 1460, size, 1)
    pay, d_cuts = torch.zeros(size + 16, dtype=torch.uint8, device="cuda"), dev(cuts)
    tmpl = torch.zeros(64, dtype=torch.uint8, device="cuda")
    hdr = torch.full((32 * n_seg + 16,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(mode=0, p=pay.data_ptr(), nbytes=size, seg=1460, tm=tmpl.data_ptr(), n=n_seg, hd=hdr.data_ptr(), off=None):
        ctx.batch_segment_headers(p, nbytes, seg, d_cuts, 1, tm, 1, n, hd, pay_off=off, mode=mode)

    for bad in (dict(mode=2), dict(p=pay.data_ptr() + 2), dict(nbytes=size + 1), dict(seg=12), dict(seg=1462),
                dict(seg=65536), dict(tm=tmpl.data_ptr() + 8), dict(hd=hdr.data_ptr() + 8), dict(hd=None),
                dict(n=(1 << 31) + 1), dict(off=hdr.data_ptr() + 4)):
        with pytest.raises(tcpck.TcpckError) as e:
            call(**bad)
        assert e.value.status == tcpck.EINVAL, bad
    call(n=0, hd=None)  # an empty ring: nothing to do
    torch.cuda.synchronize()
    assert bool((hdr == 0xA5).all().item())
