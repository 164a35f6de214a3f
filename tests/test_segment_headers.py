"""CPU tests of the send ring's planner (tcpck_plan_cuts) and of zero-copy segmentation's host twin
(tcpck_segment_headers): bit-exact against the reference's own send path (the segment_golden
fixture) and against oracle.ref16.segment_np applied per cut."""
import numpy as np
import pytest

from segment_headers_np import make_cuts, ring_np


def golden_ring(G, seg):
    """Every fixture stream in one arena, one cut per case, planned at `seg`."""
    import tcpck
    cases = G.cases
    cuts, size = make_cuts([c["payload_len"] for c in cases], [c["seq0"] for c in cases], range(len(cases)))
    payload = np.zeros(size, np.uint8)
    for cut, c in zip(cuts, cases):
        payload[int(cut["offset"]):int(cut["offset"]) + c["payload_len"]] = G.payload(c)
    tmpl = np.stack([G.template(c) for c in cases])
    return payload, cuts, tmpl, tcpck.plan_cuts(cuts, seg, size, len(cases))


def check_golden_rows(G, cases, cuts, seg, hdr, cs):
    """The cuts (one per case) whose fixture was cut at `seg`: bytes 0-31 of the reference's own images."""
    for cut, c in zip(cuts, cases):
        if c["seg"] != seg:
            continue
        f, ref, at = int(cut["first"]), G.images(c), 0
        for k, n in enumerate(c["lengths"]):
            np.testing.assert_array_equal(hdr[f + k], ref[at:at + 32], err_msg=f"{c['name']} {k}")
            at += n
        assert list(cs[f:f + len(c["lengths"])]) == c["checksums"], c["name"]


def test_plan_cuts_prefix_and_total(built_lib):
    import tcpck
    sizes = [1460, 1462, 2, 0, 1460 * 3, 0, 1460 * 130 + 2]
    cuts, size = make_cuts(sizes, [0] * 7, [0] * 7)
    cuts["first"] = 99
    assert tcpck.plan_cuts(cuts, 1460, size, 1) == 1 + 2 + 1 + 0 + 3 + 0 + 131
    assert list(cuts["first"]) == [0, 1, 3, 4, 4, 7, 7]
    assert tcpck.plan_cuts(cuts[:0].copy(), 1460, size, 1) == 0


@pytest.mark.parametrize("field,value", [("offset", 2), ("bytes", 1461), ("offset", 1 << 20), ("bytes", 1 << 20),
                                         ("tmpl", 3)])
def test_plan_cuts_rejects_and_writes_nothing(built_lib, field, value):
    import tcpck
    cuts, size = make_cuts([1460, 2920, 100], [0] * 3, [0, 1, 2])
    cuts["first"] = 99
    cuts[1][field] = value
    with pytest.raises(tcpck.TcpckError) as e:
        tcpck.plan_cuts(cuts, 1460, size, 3)
    assert e.value.status == tcpck.EINVAL and list(cuts["first"]) == [99] * 3


def test_plan_cuts_rejects_rings_above_2_31(built_lib):
    import tcpck
    cuts = np.zeros(9, tcpck.send_cut_dtype())
    cuts["bytes"] = (1 << 32) - 16  # 2^28 - 1 segments of 16 B each: eight such cuts fit, nine more segments do not
    assert tcpck.plan_cuts(cuts[:8].copy(), 16, 1 << 33, 1) == 8 * ((1 << 28) - 1)
    cuts["bytes"][8] = 16 * 9
    with pytest.raises(tcpck.TcpckError):
        tcpck.plan_cuts(cuts, 16, 1 << 33, 1)
    for seg, nbytes in ((12, 1 << 20), (18, 1 << 20), (65536, 1 << 20), (1460, (1 << 20) + 1)):
        with pytest.raises(tcpck.TcpckError):
            tcpck.plan_cuts(cuts[:1].copy(), seg, nbytes, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_host_twin_on_each_golden_case_as_one_cut(built_lib, segment_golden, mode):
    import tcpck
    G = segment_golden
    for c in G.cases:
        payload, tmpl = G.payload(c), G.template(c)[None, :]
        cuts, size = make_cuts([c["payload_len"]], [c["seq0"]], [0])
        if c["seg"] < 16:  # below the contract's smallest segment: refused, not cut
            with pytest.raises(tcpck.TcpckError):
                tcpck.plan_cuts(cuts, c["seg"], size, 1)
            continue
        n_seg = tcpck.plan_cuts(cuts, c["seg"], size, 1)
        assert n_seg == len(c["lengths"])
        hdr, off, ln, cs = tcpck.segment_headers(payload, c["seg"], cuts, tmpl, n_seg, mode)
        exp = ring_np(payload, cuts, tmpl, c["seg"], n_seg, mode)
        for got, want in zip((hdr, off, ln, cs), exp):
            np.testing.assert_array_equal(got, want, err_msg=c["name"])
        if mode == 0:
            check_golden_rows(G, [c], cuts, c["seg"], hdr, cs)
            assert list(ln + 32) == c["lengths"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seg", [16, 100, 1000, 1024, 1448, 1460, 9000, 65532])
def test_host_twin_on_the_golden_ring(built_lib, segment_golden, seg, mode):
    """All fixture streams as one ring, at every segment size a fixture was cut at."""
    import tcpck
    payload, cuts, tmpl, n_seg = golden_ring(segment_golden, seg)
    hdr, off, ln, cs = tcpck.segment_headers(payload, seg, cuts, tmpl, n_seg, mode)
    for got, want in zip((hdr, off, ln, cs), ring_np(payload, cuts, tmpl, seg, n_seg, mode)):
        np.testing.assert_array_equal(got, want)
    if mode == 0:
        check_golden_rows(segment_golden, segment_golden.cases, cuts, seg, hdr, cs)


def test_host_twin_argument_errors(built_lib):
    import tcpck
    L = tcpck.lib()
    cuts, size = make_cuts([1460 * 2], [5], [0])
    n_seg = tcpck.plan_cuts(cuts, 1460, size, 1)
    pay, tmpl = np.zeros(size + 16, np.uint8), np.zeros(64, np.uint8)
    t = tmpl.ctypes.data + (-tmpl.ctypes.data) % 16
    hdr = np.full(32 * n_seg + 16, 0xA5, np.uint8)
    h = hdr.ctypes.data + (-hdr.ctypes.data) % 16

    def call(mode=0, p=pay.ctypes.data, nbytes=size, seg=1460, tm=t, n=n_seg, hd=h):
        return L.tcpck_segment_headers(mode, p, nbytes, seg, cuts.ctypes.data, 1, tm, 1, n, hd, None, None, None)

    for bad in (dict(mode=2), dict(p=pay.ctypes.data + 2), dict(nbytes=size + 1), dict(seg=12), dict(seg=1462),
                dict(seg=65536), dict(tm=t + 8), dict(hd=h + 8), dict(hd=None), dict(n=(1 << 31) + 1)):
        assert call(**bad) == tcpck.EINVAL, bad
        assert (hdr == 0xA5).all(), bad
    assert call(n=0, hd=None) == tcpck.OK
    assert call() == tcpck.OK and not (hdr[h - hdr.ctypes.data:][:64] == 0xA5).all()
