"""GPU parity: FILL without a results buffer from concurrent callers.

The reference inserts checksums from at least three threads at once -- the
timer worker under a socket mutex (include/socket-manager.h:255-260), the
app/reaction threads through SendPacket (src/socket-manager.cc:6-11) and the
receive thread (src/network-service.cc:55-56) -- each on its own packet.  The
batched equivalent is several host threads, each on its own stream and arena,
calling OP_FILL with out=None at once: AUTO's two-pass forms then write their
results into the context's scratch slots (tcpck.h), and two FILLs sharing a
slot without ordering would store each other's checksums.  Every arena is
compared byte-exact with the reference's insert (oracle/ref16.c restating
include/tcp-header.h:252-263, pinned by tests/golden).

Also: which out-less FILLs take a slot at all (only the forms
that read the results back -- on both sides of every edge of AUTO's FILL
forms, the expectation read from the router's recorded launches,
tests/golden/router_trace.txt), and that a FILL captured into a HIP graph
takes none and replays byte-exact.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_full_paths import expected_fill  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module", params=[False, True], ids=["libtcpck", "probe"])
def any_ctx(request, built_lib):
    import tcpck
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    c = tcpck.Context(0, probe=request.param)
    yield c
    c.close()


def _c2_arena(count, seed, oracle_c):
    import tcpck
    L = 1492
    a = torch.empty(count * L, dtype=torch.uint8, device="cuda")
    tcpck.synth_fixed(a, L, L, count, seed=seed)
    want = expected_fill(host(a), np.arange(count, dtype=np.int64) * L, np.full(count, L), oracle_c)
    return a, want


def _c3_arena(count, seed, oracle_c):
    import tcpck
    import synth_np
    off, ln, total = synth_np.mixed_layout(count, seed=seed)
    a = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_off, d_ln = dev(off), dev(ln)
    tcpck.synth_var(a, d_off, d_ln, 1492, count, seed=seed)
    want = expected_fill(host(a), off, ln, oracle_c)
    hints = dict(total_bytes=int(ln.astype(np.int64).sum()), min_len=int(ln.min()), max_len=int(ln.max()),
                 packed=True)
    return a, want, d_off, d_ln, hints


@pytest.mark.parametrize("layout", ["c2", "c3"])
def test_fill_noout_four_threads_four_streams(any_ctx, oracle_c, layout):
    """4 host threads, each on its own stream and arena, 20 out-less FILLs each
    at once (FILL is idempotent: the field is zeroed before the sum), C2's
    fixed layout or C3's packed mix: every arena byte-exact."""
    import tcpck
    n_thr, reps = 4, 20
    jobs = []
    for t in range(n_thr):
        if layout == "c2":
            a, want = _c2_arena(1 << 17, 60 + t, oracle_c)
            jobs.append((a, want, None))
        else:
            a, want, d_off, d_ln, hints = _c3_arena(1 << 19, 70 + t, oracle_c)
            jobs.append((a, want, (d_off, d_ln, hints)))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(n_thr)]
    barrier = threading.Barrier(n_thr)
    errors = []

    def worker(i):
        try:
            a, _, var = jobs[i]
            s = streams[i]
            barrier.wait()
            for _ in range(reps):
                if var is None:
                    any_ctx.batch_fixed(tcpck.OP_FILL, a, 1492, 1492, a.numel() // 1492, None, stream=s)
                else:
                    d_off, d_ln, hints = var
                    any_ctx.batch_var(tcpck.OP_FILL, a, d_off, d_ln, d_off.numel(), None, stream=s, **hints)
            s.synchronize()
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(n_thr)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for a, want, _ in jobs:
        np.testing.assert_array_equal(host(a), want)


def test_scratch_taken_only_by_forms_that_read_results(built_lib, oracle_c):
    """A fresh probe context: a 128-B out-less FILL (gstream, in-stream fields)
    and a 96-B one (vvstream in-stream) allocate no slot; C2's 1492-B
    out-less FILL (rstream's deferred fields) allocates the slots and uses one;
    the bytes are the reference's insert each time."""
    import tcpck
    c = tcpck.Context(0, probe=True)
    try:
        for L in (128, 96):
            count = 50000
            a = torch.empty(count * L, dtype=torch.uint8, device="cuda")
            tcpck.synth_fixed(a, L, L, count, seed=L)
            want = expected_fill(host(a), np.arange(count, dtype=np.int64) * L, np.full(count, L), oracle_c)
            c.batch_fixed(tcpck.OP_FILL, a, L, L, count, None)
            np.testing.assert_array_equal(host(a), want)
            assert c.scratch_state() == (0, 0), L
        a, want = _c2_arena(1 << 16, 81, oracle_c)
        c.batch_fixed(tcpck.OP_FILL, a, 1492, 1492, 1 << 16, None)
        np.testing.assert_array_equal(host(a), want)
        alloc, used = c.scratch_state()
        assert alloc == 4 and bin(used).count("1") == 1
    finally:
        c.close()


def test_fill_noout_under_graph_capture(built_lib, oracle_c):
    """An out-less C2 FILL captured into a HIP graph (torch.cuda.graph) takes
    no scratch slot (its in-stream form runs instead) and the replayed graph
    stores the reference's fields."""
    import tcpck
    c = tcpck.Context(0, probe=True)
    try:
        count, L = 1 << 16, 1492
        a, want = _c2_arena(count, 82, oracle_c)
        before = c.scratch_state()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                c.batch_fixed(tcpck.OP_FILL, a, L, L, count, None, stream=torch.cuda.current_stream())
        assert c.scratch_state() == before
        tcpck.synth_fixed(a, L, L, count, seed=82)  # the capture ran nothing: restore the images anyway
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host(a), want)
        assert c.scratch_state() == before
    finally:
        c.close()


def _golden_has_field_pass(key):
    """Whether the recorded launches (tests/golden/router_trace.txt) of the
    request `key` -- with a results buffer -- include FILL's field pass."""
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, "tests", "golden", "router_trace.txt")) as f:
        lines = [l for l in f if l.startswith(key + " ->")]
    assert len(lines) == 1, key
    return " patch(" in lines[0]


def _mean_exact_lengths(count, typical, lo=30, hi=1492):
    """count even lengths in [lo, hi] with mean exactly `typical`, minimum lo
    and maximum hi: all `typical`, but one image of lo and one of hi, and the
    bytes that pair is off the mean by spread over the next images."""
    ln = np.full(count, typical, np.int64)
    ln[0], ln[1] = lo, hi
    k, d = 2, 2 * typical - lo - hi  # bytes still to add (d > 0) or to take away
    while d:
        step = min(d, hi - typical) if d > 0 else max(d, lo - typical)
        ln[k] += step
        d -= step
        k += 1
    assert ln.min() == lo and ln.max() == hi and int(ln.sum()) == count * typical and not (ln & 1).any()
    return ln.astype(np.uint32)


def test_scratch_exactly_where_the_plan_has_a_field_pass(built_lib, oracle_c):
    """Both sides of every edge of AUTO's FILL forms, out-less through
    batch_*_ex with KERNEL_AUTO, each on a fresh (probe library: scratch_state)
    context and 4,096 images, with param 0 and TCPCK_PARAM_FILL_INSTREAM:
    packed fixed images of 318 / 320 B (vvstream's deferred form from 320 B)
    and 512 / 1024 B (vvstream deferred / rstream 25), 510 / 512-B images in
    2048-B slots (sstream's deferred form from 512 B), a packed offset list of
    typical image 446 / 450 B (the update form from 448 B), and in RFC 1071
    mode of 1022 / 1026 B (vvstream's deferred form from 1 KiB; REF batches of
    that size take the update form).  The arena is the oracle's FILL byte for
    byte, and a scratch slot is used exactly when the recorded launches of the
    same request with a results buffer have a field pass -- the expectation is
    read from the router's golden trace, not restated here."""
    import tcpck
    count = 4096
    cases = [("fixed", L, st, tcpck.MODE_REF) for L, st in
             ((318, 318), (320, 320), (512, 512), (1024, 1024), (510, 2048), (512, 2048))]
    cases += [("var", t, 0, tcpck.MODE_REF) for t in (446, 450)]
    cases += [("var", t, 0, tcpck.MODE_RFC1071) for t in (1022, 1026)]
    seen = set()
    for kind, L, stride, mode in cases:
        for param in (0, tcpck.PARAM_FILL_INSTREAM):
            mname = "REF" if mode == tcpck.MODE_REF else "RFC"
            if kind == "fixed":
                key = f"F op=FILL mode={mname} out=1 hdr=0 n=1000 al=0 len={L} st={stride} k=AUTO p={param:#x} hk=0"
                off = np.arange(count, dtype=np.int64) * stride
                ln = np.full(count, L, np.uint32)
                a = torch.zeros(count * stride, dtype=torch.uint8, device="cuda")
                tcpck.synth_fixed(a, stride, L, count, seed=L)
            else:
                key = (f"V op=FILL mode={mname} out=1 hdr=0 n=1000 al=0 lay=P typ={L} min=30 max=1492 base=0 "
                       f"k=AUTO p={param:#x} hk=0")
                ln = _mean_exact_lengths(count, L)
                off = np.concatenate(([0], np.cumsum(ln.astype(np.int64))[:-1]))
                a = torch.zeros(count * L, dtype=torch.uint8, device="cuda")
                d_off, d_ln = dev(off.astype(np.uint64)), dev(ln)
                tcpck.synth_var(a, d_off, d_ln, 1492, count, seed=L)
            assert a.data_ptr() % 16 == 0
            field_pass = _golden_has_field_pass(key)
            seen.add(field_pass)
            want = expected_fill(host(a), off, ln, oracle_c, mode=mode)
            c = tcpck.Context(0, probe=True)
            try:
                if kind == "fixed":
                    c.batch_fixed_ex(tcpck.OP_FILL, a, stride, L, count, None, tcpck.KERNEL_AUTO, param, mode=mode)
                else:
                    c.batch_var_ex(tcpck.OP_FILL, a, d_off, d_ln, count, None, tcpck.KERNEL_AUTO, param, mode=mode,
                                   total_bytes=count * L, min_len=30, max_len=1492, packed=True)
                np.testing.assert_array_equal(host(a), want, err_msg=key)
                alloc, used = c.scratch_state()
                print(key, "field pass" if field_pass else "in-stream", (alloc, used))
                assert (used != 0) == field_pass and alloc == (4 if field_pass else 0), (key, alloc, used)
            finally:
                c.close()
    assert seen == {False, True}
