"""tcpck -- Python binding of libtcpck.so (the MI355X TCP checksum library).

A thin ctypes layer over the C ABI declared in include/tcpck.h, used by the
parity tests and bench.py.  There is no Python or CPU fallback for the batched
path: if libtcpck.so is missing or the device is not a gfx950, constructing a
``Context`` raises.

libtcpck.so holds the kernels the AUTO policy can pick; its tcpck_tuning.h
entry points (``batch_*_ex``) accept only those.  ``Context(probe=True)``
binds libtcpck_probe.so instead: the same sources built with every measured
variant, the per-wave time stamps and the diag kernels (scripts/, the
variant tests).

Reference API mirrored (filixi/TCP-stack):
  * ``checksum16``   <- CalculateChecksum(const TcpPacket&), include/tcp-header.h:252-263
  * OP_FILL          <- Checksum()=0; Checksum()=CalculateChecksum(pkt),
                        src/socket-manager.cc:9-10, include/socket-manager.h:259-260
  * OP_VERIFY        <- CalculateChecksum(pkt) == 0, include/socket-manager.h:182
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(PKG_ROOT, "libtcpck.so")
# tests/test_abi_asan.py only: the same product library with its host code
# built under ASan + UBSan (tcp-stack_amd/Makefile `asan`), loaded in place of
# libtcpck.so by a python started with the sanitizer runtime preloaded
ASAN_PATH = os.path.join(PKG_ROOT, "libtcpck_asan.so")
if os.environ.get("TCPCK_LIB_VARIANT") == "asan":
    LIB_PATH = ASAN_PATH
PROBE_PATH = os.path.join(PKG_ROOT, "libtcpck_probe.so")

OK = 0
EINVAL = -22
ENOMEM = -12
ENODEV = -19
EHIP = -1000

MODE_REF = 0
MODE_RFC1071 = 1

OP_CHECKSUM = 0
OP_FILL = 1
OP_VERIFY = 2
OP_RECEIVE = 3  # VERIFY + TcpHeaderN2H in place (device batches)
HEADER_BYTES = 32

LAYOUT_PACKED = 1
LAYOUT_SORTED = 2

# receive delivery (tcpck_batch_deliver / tcpck_plan_deliver)
DELIVER_SKIP = 0xFFFFFFFFFFFFFFFF  # dst[k]: image k is not delivered
RCV_ACCEPT = 1    # Estab's data/ACK branch took the image
RCV_PAYLOAD = 2   # ... and Accept() appends its payload (dst[k] set)
RCV_SEND_ACK = 4  # the reference replies SendAck(snd_nxt, ack[k], .)
RCV_BAD_SUM = 8   # checksum failed: InvalideCheckSum(), Discard + SendAck

# receive demultiplex (tcpck_conn_table_* / tcpck_batch_demux / tcpck_plan_deliver_multi)
CONN_NONE = 0xFFFFFFFF  # no entry for the image's key
CONN_ESTAB = 0    # ConnState.flags: planned by Estab's rule
CONN_HOST = 1     # ... every image goes to the host state machine
NOT_STOPPED = 0xFFFFFFFFFFFFFFFF  # ConnState.stopped_at: the connection's walk ran to the end of the ring
RCV_RST = 16      # no socket, good sum: reply RST, seq = ack[k] (the image's ack number)
RCV_HOST = 32     # not decided here: the host path takes the image, in arrival order
REPLY_BYTES = 32  # one reply of tcpck_batch_reply / tcpck_build_replies: a header, no payload

# batched resend pass (tcpck_batch_resend / tcpck_resend_images)
SND_CLOSED = 1     # SndState.flags: state_.GetState() == State::kClosed
RESEND_REF = 0     # the reference's compare (socket-internal.h:381-385), bit for bit
RESEND_SERIAL = 1  # opt-in: RFC 793 serial arithmetic

# include/tcpck_tuning.h
KERNEL_AUTO = 0
KERNEL_SEG = 1    # param: seg shape + 1 (1..11, SEG_SHAPES), 0 = by length
KERNEL_RSTREAM = 5  # fixed stride == len: param = variant (10 = policy) | cap << 8 | oversub << 16
KERNEL_VVSTREAM = 8  # packed variable or fixed (stride >= len): param = 0/1 U4/U8 byte split, 2/3 count split, 4 policy | oversub << 16
KERNEL_GSTREAM = 9  # fixed stride == len, len a power of two in [32, 1024], 16-B aligned arena: param = 0/1/2 U4/U8/U2 (+4 default block order) | oversub << 16
KERNEL_PATCH = 12  # libtcpck_probe.so only (tcpck_probe.h): FILL's deferred field pass alone
KERNEL_SSTREAM = 10  # slotted layouts (fixed slots, stride % 16 == 0, or any offset list): param = 0 policy (U4, scattered order), 1 U4, 2 U8 (+4 default block order, +8 scattered) | oversub << 16
KERNEL_RVSTREAM = 13  # packed offset lists, REF, CHECKSUM / VERIFY: rstream's scalar walk over the lengths
SEG_SHAPES = {1: "G8/U2", 2: "G16/U6", 3: "G64/U4", 4: "G64/U2", 5: "G32/U3", 6: "G4/U8", 7: "W4/U4", 8: "W8/U4", 9: "W16/U2", 10: "W16/U4", 11: "W2/U4"}
# include/tcpck_tuning.h: in libtcpck.so (AUTO's kernels only) and libtcpck_probe.so
TUNING_EXPORTS = ("tcpck_batch_fixed_ex", "tcpck_batch_var_ex", "tcpck_batch_segment_ex", "tcpck_batch_receive_ex")
# include/tcpck_tuning.h, measurement only: libtcpck_probe.so
PROBE_EXPORTS = ("tcpck_ctx_set_debug", "tcpck_diag_stream", "tcpck_probe_receive_ex", "tcpck_probe_scratch_state",
                 "tcpck_probe_scratch_fail", "tcpck_probe_set_fill_pipe", "tcpck_probe_set_deliver_grid")
# include/tcpck_probe.h: tcpck_probe_receive_ex's flags word (the header pass forms)
PROBE_RECEIVE_HDR_FIRST = 1    # accepted, no effect (the product's separate header pass runs first since round 5)
PROBE_PARAM_PATCH_REVERSE = 1 << 27  # tcpck_batch_*_ex param (probe library): FILL's field pass in reverse order
PROBE_PIPE_ONE_STREAM = 0x100  # set_fill_pipe(k | this): the k chunks on the caller's stream only
PROBE_RECEIVE_HDR_AFTER = 16   # the separate header pass after VERIFY (the order before round 5)
PROBE_RECEIVE_CONCURRENT = 2   # header pass on a side stream beside VERIFY
PROBE_RECEIVE_HDR_WT = 4       # header array stores written through
PROBE_RECEIVE_HDR_WIDE = 8     # two lanes per image, 16-B loads with cache bits (flags >> 4) & 3
PROBE_RECEIVE_ORDER_SHIFT = 8  # (flags >> 8) & 3: header pass image order (1 XCD-chunked, 2 scattered, 3 transposed)
# Kernel params libtcpck.so runs (the AUTO policy's own choices, tcpck_plan.cc
# plan_fixed / plan_var); every other value needs libtcpck_probe.so.
SEG_AUTO_SHAPES = (0, 1, 2, 7, 8, 9, 11)  # by length, G8/U2, G16/U6, W4, W8, W16, W2 (shape_for_len)
RSTREAM_AUTO = (20, 25)                   # the policy; 25: its FILL with the write-through 2-B field pass
GSTREAM_AUTO = (0, 0x80, 0x401)           # (+ 4: default block order)
SSTREAM_AUTO = (0, 32, 128)               # the policy; + 32: RECEIVE headers from the stream; + 128: FILL's deferred fields


def in_product(kernel: int, param: int, op: int | None = None) -> bool:
    """Whether libtcpck.so runs `kernel` with `param` (tcpck_tuning.h) for `op`."""
    if kernel == KERNEL_AUTO:
        return True
    if kernel == KERNEL_PATCH:
        return False
    if kernel == KERNEL_SEG:
        return (param & 0xFF) in SEG_AUTO_SHAPES
    if kernel == KERNEL_RSTREAM:
        return (param & 0xFF) in RSTREAM_AUTO
    if kernel == KERNEL_VVSTREAM:
        return (param & 7) == 4
    if kernel == KERNEL_GSTREAM:  # AUTO's FILL only
        return (param & 0xFFFF & ~4) in GSTREAM_AUTO and op in (None, OP_FILL)
    if kernel == KERNEL_SSTREAM:
        return (param & 0xFF) in SSTREAM_AUTO
    return True  # unknown kernels: both libraries reject them


def segment_in_product(param: int) -> bool:
    """Whether libtcpck.so runs tcpck_batch_segment_ex with `param` (0: the policy; + 8: default order)."""
    return (param & 7) == 0


PARAM_FILL_UPDATE = 1 << 28  # FILL: the kernel's CHECKSUM pass + the field-update pass
PARAM_FILL_INSTREAM = 1 << 29  # FILL under AUTO: the field zeroed in the stream
PARAM_RECEIVE_TWO_PASS = 1 << 30  # RECEIVE into a header array: separate header pass

# Every symbol include/tcpck.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "tcpck_abi_version", "tcpck_strerror", "tcpck_device_supported",
    "tcpck_ctx_create", "tcpck_ctx_destroy", "tcpck_ctx_device",
    "tcpck_checksum16", "tcpck_fill16", "tcpck_update16",
    "tcpck_batch_fixed", "tcpck_batch_var", "tcpck_batch_set_ack",
    "tcpck_host_batch_fixed", "tcpck_host_batch_var", "tcpck_ctx_set_chunk_bytes",
    "tcpck_host_alloc", "tcpck_host_free", "tcpck_device_alloc", "tcpck_device_free",
    "tcpck_memcpy_h2d", "tcpck_memcpy_d2h", "tcpck_stream_sync",
    "tcpck_synth_fixed", "tcpck_synth_var", "tcpck_batch_segment", "tcpck_batch_header_swap",
    "tcpck_batch_receive", "tcpck_host_batch_fixed_multi", "tcpck_host_batch_var_multi",
    "tcpck_batch_deliver", "tcpck_plan_deliver",
    "tcpck_conn_table_create", "tcpck_conn_table_destroy", "tcpck_conn_table_set", "tcpck_conn_table_erase",
    "tcpck_conn_table_find", "tcpck_conn_table_commit", "tcpck_conn_table_stats", "tcpck_batch_demux",
    "tcpck_plan_deliver_multi",
    "tcpck_reply_scratch_bytes", "tcpck_batch_reply", "tcpck_build_replies",
    "tcpck_resend_scratch_bytes", "tcpck_batch_resend", "tcpck_resend_images",
)


class TcpckError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: status {status} ({strerror(status)})")


class Layout(ctypes.Structure):
    _fields_ = [("total_bytes", ctypes.c_uint64), ("min_len", ctypes.c_uint32),
                ("max_len", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class RcvState(ctypes.Structure):
    """tcpck_rcv_state: the TcpControlBlock fields Estab reads and writes, and the
    bytes appended to the receive stream so far."""
    _fields_ = [("rcv_nxt", ctypes.c_uint32), ("snd_nxt", ctypes.c_uint32), ("snd_una", ctypes.c_uint32),
                ("rcv_wnd", ctypes.c_uint16), ("reserved", ctypes.c_uint16), ("delivered", ctypes.c_uint64)]


class ConnState(ctypes.Structure):
    """tcpck_conn_state: one connection of a mixed ring for plan_deliver_multi -- its control
    block, its window [recv_base, recv_base + recv_bytes) of the shared receive buffer, where
    its walk stopped (out) and CONN_ESTAB / CONN_HOST."""
    _fields_ = [("rcv", RcvState), ("recv_base", ctypes.c_uint64), ("recv_bytes", ctypes.c_uint64),
                ("stopped_at", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SndState(ctypes.Structure):
    """tcpck_snd_state: what ResendPredicate reads of a connection (socket-internal.h:363-390):
    snd_una, rcv_nxt and SND_CLOSED in flags.  16 bytes; a numpy table of them is uint32[n, 4]."""
    _fields_ = [("snd_una", ctypes.c_uint32), ("rcv_nxt", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


_libs: dict = {}


def lib(probe: bool = False) -> ctypes.CDLL:
    """Loads libtcpck.so (probe: libtcpck_probe.so), built in-tree by
    __graft_entry__.build(); raises if absent."""
    if probe in _libs:
        return _libs[probe]
    path = PROBE_PATH if probe else LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    vp, u64, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    sig = {
        "tcpck_abi_version": (i32, []),
        "tcpck_strerror": (ctypes.c_char_p, [i32]),
        "tcpck_device_supported": (i32, [i32]),
        "tcpck_ctx_create": (i32, [i32, ctypes.POINTER(vp)]),
        "tcpck_ctx_destroy": (i32, [vp]),
        "tcpck_ctx_device": (i32, [vp]),
        "tcpck_checksum16": (i32, [vp, sz, i32, ctypes.POINTER(ctypes.c_uint16)]),
        "tcpck_fill16": (i32, [vp, sz, i32, ctypes.POINTER(ctypes.c_uint16)]),
        "tcpck_update16": (ctypes.c_uint16, [ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint16, i32]),
        "tcpck_batch_fixed": (i32, [vp, i32, i32, vp, u64, u32, u64, vp, vp]),
        "tcpck_batch_var": (i32, [vp, i32, i32, vp, vp, vp, u64, vp, ctypes.POINTER(Layout), vp]),
        "tcpck_batch_set_ack": (i32, [vp, i32, vp, vp, u64, u64, vp, u32, vp, vp]),
        "tcpck_host_batch_fixed": (i32, [vp, i32, i32, vp, u64, u32, u64, vp]),
        "tcpck_host_batch_var": (i32, [vp, i32, i32, vp, vp, vp, u64, vp]),
        "tcpck_host_batch_fixed_multi": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, u64, u32, u64, vp]),
        "tcpck_host_batch_var_multi": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, vp, vp, u64, vp]),
        "tcpck_ctx_set_chunk_bytes": (i32, [vp, u64]),
        "tcpck_host_alloc": (i32, [sz, ctypes.POINTER(vp)]),
        "tcpck_host_free": (i32, [vp]),
        "tcpck_device_alloc": (i32, [vp, sz, ctypes.POINTER(vp)]),
        "tcpck_device_free": (i32, [vp, vp]),
        "tcpck_memcpy_h2d": (i32, [vp, vp, vp, sz]),
        "tcpck_memcpy_d2h": (i32, [vp, vp, vp, sz]),
        "tcpck_stream_sync": (i32, [vp, vp]),
        "tcpck_synth_fixed": (i32, [vp, u64, u32, u64, u64, u64, i32, vp]),
        "tcpck_synth_var": (i32, [vp, vp, vp, u32, u64, u64, u64, i32, vp]),
        "tcpck_batch_segment": (i32, [vp, i32, vp, u64, u32, vp, u32, vp, u64, vp, vp]),
        "tcpck_batch_segment_ex": (i32, [vp, i32, vp, u64, u32, vp, u32, vp, u64, vp, i32, vp]),
        "tcpck_batch_header_swap": (i32, [vp, vp, vp, u64, u64, vp]),
        "tcpck_batch_receive": (i32, [vp, i32, vp, u64, u32, vp, vp, u64, vp, vp, ctypes.POINTER(Layout), vp]),
        "tcpck_batch_receive_ex": (i32, [vp, i32, vp, u64, u32, vp, vp, u64, vp, vp, ctypes.POINTER(Layout), i32, i32,
                                         vp]),
        "tcpck_batch_deliver": (i32, [vp, vp, u64, u32, vp, vp, u64, vp, vp, u64, vp]),
        "tcpck_plan_deliver": (i32, [vp, vp, vp, u32, u64, ctypes.POINTER(RcvState), u64, vp, vp, vp,
                                     ctypes.POINTER(u64)]),
        "tcpck_conn_table_create": (i32, [vp, u32, ctypes.POINTER(vp)]),
        "tcpck_conn_table_destroy": (i32, [vp]),
        "tcpck_conn_table_set": (i32, [vp, ctypes.c_uint16, u32, ctypes.c_uint16, u32]),
        "tcpck_conn_table_erase": (i32, [vp, ctypes.c_uint16, u32, ctypes.c_uint16]),
        "tcpck_conn_table_find": (i32, [vp, ctypes.c_uint16, u32, ctypes.c_uint16, ctypes.POINTER(u32)]),
        "tcpck_conn_table_commit": (i32, [vp, vp]),
        "tcpck_conn_table_stats": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32),
                                         ctypes.POINTER(u64)]),
        "tcpck_batch_demux": (i32, [vp, vp, vp, u64, vp, vp]),
        "tcpck_plan_deliver_multi": (i32, [vp, vp, vp, vp, u32, u64, ctypes.POINTER(ConnState), u32, vp, vp, vp]),
        "tcpck_reply_scratch_bytes": (i32, [u64, ctypes.POINTER(sz)]),
        "tcpck_batch_reply": (i32, [vp, i32, vp, vp, vp, vp, u32, u64, vp, u64, vp, vp, vp, vp]),
        "tcpck_build_replies": (i32, [i32, vp, vp, vp, vp, u32, u64, vp, u64, vp, ctypes.POINTER(u64)]),
        "tcpck_resend_scratch_bytes": (i32, [u64, ctypes.POINTER(sz)]),
        "tcpck_batch_resend": (i32, [vp, i32, i32, vp, u64, u64, u32, vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp, u64,
                                     vp, vp, vp]),
        "tcpck_resend_images": (i32, [i32, i32, vp, u64, u64, u32, vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp, u64,
                                      ctypes.POINTER(u64)]),
        # include/tcpck_tuning.h
        "tcpck_batch_fixed_ex": (i32, [vp, i32, i32, vp, u64, u32, u64, vp, i32, i32, vp]),
        "tcpck_batch_var_ex": (i32, [vp, i32, i32, vp, vp, vp, u64, vp, ctypes.POINTER(Layout), i32, i32, vp]),
        "tcpck_ctx_set_debug": (i32, [vp, vp]),
        "tcpck_probe_scratch_state": (i32, [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "tcpck_probe_scratch_fail": (i32, [vp, i32, ctypes.POINTER(u64)]),
        "tcpck_probe_set_fill_pipe": (i32, [vp, i32, i32]),
        "tcpck_probe_set_deliver_grid": (i32, [vp, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                               ctypes.POINTER(u64)]),
        "tcpck_diag_stream": (i32, [vp, i32, vp, u64, vp, vp]),
        "tcpck_probe_receive_ex": (i32, [vp, i32, vp, u64, u32, vp, vp, u64, vp, vp, ctypes.POINTER(Layout), i32, i32,
                                         i32, vp]),
    }
    for name, (res, args) in sig.items():
        if name in PROBE_EXPORTS and not probe:
            continue  # measurement-only: not in the product library
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _libs[probe] = L
    return L


def probe_lib() -> ctypes.CDLL:
    """libtcpck_probe.so (every measured kernel variant; tcpck_tuning.h in full)."""
    return lib(probe=True)


def strerror(status: int) -> str:
    try:
        return lib().tcpck_strerror(status).decode()
    except ImportError:
        return "libtcpck.so unavailable"


def _check(status: int, what: str) -> None:
    if status != OK:
        raise TcpckError(status, what)


def _ptr(x) -> int | None:
    """Device/host address of a torch tensor, numpy array or int (None -> NULL)."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    raise TypeError(f"cannot take the address of {type(x)}")


def _stream(s) -> int | None:
    if s is None:
        return None
    if isinstance(s, int):
        return s
    return s.cuda_stream  # torch.cuda.Stream


# ---- single image, host ------------------------------------------------------

def _as_u8(buf):
    import numpy as np
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(buf), dtype=np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8)


def checksum16(buf, mode: int = MODE_REF) -> int:
    """CalculateChecksum of one host image (tcp-header.h:252-263)."""
    a = _as_u8(buf)
    out = ctypes.c_uint16()
    _check(lib().tcpck_checksum16(a.ctypes.data, a.size, mode, ctypes.byref(out)), "tcpck_checksum16")
    return out.value


def fill16(img, mode: int = MODE_REF) -> int:
    """Send-side insertion in place on a writable uint8 numpy image."""
    out = ctypes.c_uint16()
    _check(lib().tcpck_fill16(img.ctypes.data, img.size, mode, ctypes.byref(out)), "tcpck_fill16")
    return out.value


def update16(checksum: int, old_word: int, new_word: int, mode: int = MODE_REF) -> int:
    return int(lib().tcpck_update16(checksum, old_word, new_word, mode))


def synth_fixed(arena, stride: int, length: int, count: int, seed: int = 42,
                first_index: int = 0, kind: int = 0, stream=None) -> None:
    """Fills a device arena with a fixed-stride synthetic batch (see include/tcpck.h)."""
    _check(lib().tcpck_synth_fixed(_ptr(arena), stride, length, count, seed, first_index, kind,
                                   _stream(stream)), "tcpck_synth_fixed")


def synth_var(arena, offsets, lengths, max_len: int, count: int, seed: int = 42,
              first_index: int = 0, kind: int = 0, stream=None) -> None:
    _check(lib().tcpck_synth_var(_ptr(arena), _ptr(offsets), _ptr(lengths), max_len, count, seed,
                                 first_index, kind, _stream(stream)), "tcpck_synth_var")


def plan_deliver(hdr, ok, state: RcvState, recv_bytes: int, lengths=None, length: int = 0):
    """tcpck_plan_deliver on numpy arrays (host only, no device): hdr = 32 B of host-order header
    per image as batch_receive writes them, ok = its verdicts, lengths (or one `length`) = the image
    lengths.  Walks the arrival sequence as RecvPacket + Estab do (socket-internal.h:161-171,
    state.cc:195-223), updates `state` in place and returns (dst u64[n], verdict u8[n], ack u32[n],
    consumed): dst[k] is where batch_deliver puts image k's payload, or DELIVER_SKIP."""
    import numpy as np
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    n = ok.size
    hdr = np.ascontiguousarray(hdr, dtype=np.uint8).reshape(-1)
    if hdr.size != 32 * n:
        raise ValueError("hdr must hold 32 bytes per image")
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if lengths.size != n:
            raise ValueError("lengths must hold one entry per image")
    dst = np.empty(n, np.uint64)
    verdict = np.empty(n, np.uint8)
    ack = np.empty(n, np.uint32)
    consumed = ctypes.c_uint64()
    _check(lib().tcpck_plan_deliver(hdr.ctypes.data, ok.ctypes.data, _ptr(lengths), length, n, ctypes.byref(state),
                                    recv_bytes, dst.ctypes.data, verdict.ctypes.data, ack.ctypes.data,
                                    ctypes.byref(consumed)), "tcpck_plan_deliver")
    return dst, verdict, ack, consumed.value


def plan_deliver_multi(hdr, ok, conn, conns, lengths=None, length: int = 0):
    """tcpck_plan_deliver_multi on numpy arrays (host only): plan_deliver over a ring that mixes
    connections.  conn = batch_demux's ids (CONN_NONE or an index into conns), conns = a ctypes
    array (ConnState * n) or a list of ConnState, updated in place (rcv, stopped_at).  Returns
    (dst u64[n], verdict u8[n], ack u32[n]): dst is absolute in the shared receive buffer and feeds
    one batch_deliver over the whole ring."""
    import numpy as np
    ok = np.ascontiguousarray(ok, dtype=np.uint8)
    n = ok.size
    hdr = np.ascontiguousarray(hdr, dtype=np.uint8).reshape(-1)
    conn = np.ascontiguousarray(conn, dtype=np.uint32)
    if hdr.size != 32 * n or conn.size != n:
        raise ValueError("hdr must hold 32 bytes and conn one entry per image")
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if lengths.size != n:
            raise ValueError("lengths must hold one entry per image")
    arr = conns if isinstance(conns, ctypes.Array) else (ConnState * len(conns))(*conns)
    dst = np.empty(n, np.uint64)
    verdict = np.empty(n, np.uint8)
    ack = np.empty(n, np.uint32)
    status = lib().tcpck_plan_deliver_multi(hdr.ctypes.data, ok.ctypes.data, conn.ctypes.data, _ptr(lengths), length, n,
                                            arr, len(arr), dst.ctypes.data, verdict.ctypes.data, ack.ctypes.data)
    _check(status, "tcpck_plan_deliver_multi")
    if arr is not conns:  # a list: its elements were copied into the array
        for i, c in enumerate(conns):
            ctypes.memmove(ctypes.byref(c), ctypes.byref(arr[i]), ctypes.sizeof(ConnState))
    return dst, verdict, ack


def reply_scratch_bytes(count: int) -> int:
    """Bytes of device scratch Context.batch_reply needs for a ring of `count` images (never 0)."""
    out = ctypes.c_size_t()
    _check(lib().tcpck_reply_scratch_bytes(count, ctypes.byref(out)), "tcpck_reply_scratch_bytes")
    return out.value


def build_replies(verdict, ack, tmpl, conn=None, reply_cap: int | None = None, mode: int = MODE_REF):
    """tcpck_build_replies on numpy arrays (host only, no device): the ACK / RST datagrams the
    reference sends back for a planned ring (SendAck, socket-internal.h:293-299; the RST of a datagram
    of no socket, socket-manager.h:201-207).  verdict / ack: the planner's outputs; conn: the demux
    ids (None: every image is connection 0); tmpl: 32 B of network-order header per connection (seq =
    snd_nxt, window = snd_wnd).  Returns (replies u8[written, 32], src u32[written], total): dense, in
    ring order, src[j] the image reply j answers; written = min(total, reply_cap) (reply_cap None: the
    image count)."""
    import numpy as np
    verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
    n = verdict.size
    ack = np.ascontiguousarray(ack, dtype=np.uint32)
    tmpl = np.ascontiguousarray(tmpl, dtype=np.uint8).reshape(-1)
    if ack.size != n or tmpl.size % 32:
        raise ValueError("ack must hold one entry per image and tmpl 32 bytes per connection")
    if conn is not None:
        conn = np.ascontiguousarray(conn, dtype=np.uint32)
        if conn.size != n:
            raise ValueError("conn must hold one entry per image")
    cap = n if reply_cap is None else reply_cap
    replies = np.zeros((cap + 1) * 32, np.uint8)  # (one record more: never an empty array's NULL)
    src = np.zeros(cap + 1, np.uint32)
    total = ctypes.c_uint64()
    _check(lib().tcpck_build_replies(mode, verdict.ctypes.data, ack.ctypes.data, _ptr(conn), tmpl.ctypes.data if tmpl.size
                                     else None, tmpl.size // 32, n, replies.ctypes.data, cap, src.ctypes.data,
                                     ctypes.byref(total)), "tcpck_build_replies")
    written = min(total.value, cap)
    return replies[:32 * written].reshape(-1, 32), src[:written], total.value


def resend_scratch_bytes(count: int) -> int:
    """Bytes of device scratch Context.batch_resend needs for a queue of `count` images (never 0)."""
    out = ctypes.c_size_t()
    _check(lib().tcpck_resend_scratch_bytes(count, ctypes.byref(out)), "tcpck_resend_scratch_bytes")
    return out.value


def resend_images(arena, snd, count: int | None = None, stride: int = 0, length: int = 0, offsets=None, lengths=None,
                  conn=None, out_cap: int | None = None, rule: int = RESEND_REF, mode: int = MODE_REF):
    """tcpck_resend_images on numpy arrays (host only, no device): the reference's resend event
    (ResendPredicate, socket-internal.h:363-390) over a whole send queue.  arena: writable uint8, the
    kept images are patched in place (ACK number := htonl(rcv_nxt), checksum updated).  snd: uint32[n_conns,
    4] rows of (snd_una, rcv_nxt, flags, reserved); conn: uint32 ids (None: every image is connection 0).
    Fixed layout (count, stride, length) or offsets + lengths.  Returns (keep u8[count], out_offsets
    u64[w], out_lengths u32[w], out_conn u32[w], src u32[w], total): the survivors dense and in queue
    order, w = min(total, out_cap) (out_cap None: the image count)."""
    import numpy as np
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        n = offsets.size
        if lengths.size != n:
            raise ValueError("lengths must hold one entry per image")
    else:
        n = int(count)
    snd = np.ascontiguousarray(snd, dtype=np.uint32).reshape(-1, 4)
    if conn is not None:
        conn = np.ascontiguousarray(conn, dtype=np.uint32)
        if conn.size != n:
            raise ValueError("conn must hold one entry per image")
    if not (arena.dtype == np.uint8 and arena.flags.c_contiguous and arena.flags.writeable):
        raise ValueError("arena must be a writable contiguous uint8 array")
    cap = n if out_cap is None else out_cap
    keep = np.zeros(n + 1, np.uint8)  # (one element more: never an empty array's NULL)
    out_off, out_len = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint32)
    out_conn, src = np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32)
    total = ctypes.c_uint64()
    _check(lib().tcpck_resend_images(mode, rule, arena.ctypes.data, arena.size, stride, length, _ptr(offsets),
                                     _ptr(lengths), _ptr(conn), snd.ctypes.data if snd.size else None, snd.shape[0], n,
                                     keep.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, out_conn.ctypes.data,
                                     src.ctypes.data, cap, ctypes.byref(total)), "tcpck_resend_images")
    w = min(total.value, cap)
    return keep[:n], out_off[:w], out_len[:w], out_conn[:w], src[:w], total.value


class ConnTable:
    """tcpck_conn_table: ReceivePacket's socket map (socket-manager.h:187-196, 235-245) as a host
    mirror plus a device image batch_demux probes.  Keys are (host_port, peer_ip, peer_port), a
    listener is (host_port, 0, 0); ids are the caller's (for plan_deliver_multi: indices into its
    conns).  ctx None: a host-only table (no device; batch_demux refuses it)."""

    def __init__(self, ctx, max_conns: int):
        self._L = ctx._L if ctx is not None else lib()
        self._h = ctypes.c_void_p()
        _check(self._L.tcpck_conn_table_create(ctx._h if ctx is not None else None, max_conns, ctypes.byref(self._h)),
               "tcpck_conn_table_create")
        self._ctx = ctx  # the context outlives the table
        self.max_conns = max_conns

    def set(self, host_port: int, peer_ip: int, peer_port: int, id: int) -> None:
        _check(self._L.tcpck_conn_table_set(self._h, host_port, peer_ip, peer_port, id), "tcpck_conn_table_set")

    def erase(self, host_port: int, peer_ip: int, peer_port: int) -> None:
        _check(self._L.tcpck_conn_table_erase(self._h, host_port, peer_ip, peer_port), "tcpck_conn_table_erase")

    def find(self, host_port: int, peer_ip: int, peer_port: int) -> int:
        """The key's id in the host mirror, or CONN_NONE."""
        out = ctypes.c_uint32()
        _check(self._L.tcpck_conn_table_find(self._h, host_port, peer_ip, peer_port, ctypes.byref(out)),
               "tcpck_conn_table_find")
        return out.value

    def commit(self, stream=None) -> None:
        """Rebuilds the image from the mirror and uploads it on `stream` (blocks until done)."""
        _check(self._L.tcpck_conn_table_commit(self._h, _stream(stream)), "tcpck_conn_table_commit")

    def stats(self):
        """(slots, entries, longest_probe, wrapped) of the image as last committed."""
        s, e, w, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        _check(self._L.tcpck_conn_table_stats(self._h, ctypes.byref(s), ctypes.byref(e), ctypes.byref(p),
                                              ctypes.byref(w)), "tcpck_conn_table_stats")
        return s.value, e.value, p.value, w.value

    def close(self) -> None:
        if self._h:
            self._L.tcpck_conn_table_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- context -------------------------------------------------------------------

class Context:
    """One libtcpck context bound to a HIP device (gfx950 only)."""

    def __init__(self, device: int = 0, probe: bool = False):
        self._h = ctypes.c_void_p()
        self._L = lib(probe)
        self.probe = probe
        _check(self._L.tcpck_ctx_create(device, ctypes.byref(self._h)), f"tcpck_ctx_create({device})")
        self.device = device

    def close(self) -> None:
        if self._h:
            self._L.tcpck_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # device-resident batches (the hot path)
    def batch_fixed(self, op: int, arena, stride: int, length: int, count: int, out,
                    mode: int = MODE_REF, stream=None) -> None:
        _check(self._L.tcpck_batch_fixed(self._h, op, mode, _ptr(arena), stride, length, count,
                                       _ptr(out), _stream(stream)), "tcpck_batch_fixed")

    def batch_var(self, op: int, arena, offsets, lengths, count: int, out, mode: int = MODE_REF,
                  total_bytes: int = 0, min_len: int = 0, max_len: int = 0, packed: bool = False,
                  sorted: bool = False, stream=None) -> None:
        lay = Layout(total_bytes, min_len, max_len,
                     (LAYOUT_PACKED if packed else 0) | (LAYOUT_SORTED if sorted else 0), 0)
        _check(self._L.tcpck_batch_var(self._h, op, mode, _ptr(arena), _ptr(offsets), _ptr(lengths),
                                     count, _ptr(out), ctypes.byref(lay), _stream(stream)),
               "tcpck_batch_var")

    def batch_set_ack(self, arena, count: int, ack: int = 0, acks=None, offsets=None, stride: int = 0,
                      out=None, mode: int = MODE_REF, stream=None) -> None:
        """Retransmit batch (socket-internal.h:376-377 + socket-manager.cc:9-10): bytes 20-23 of every
        image := htonl(ack or acks[k]), checksum at 28-29 updated incrementally (tcpck_batch_set_ack)."""
        _check(self._L.tcpck_batch_set_ack(self._h, mode, _ptr(arena), _ptr(offsets), stride, count,
                                         _ptr(acks), ack & 0xFFFFFFFF, _ptr(out), _stream(stream)),
               "tcpck_batch_set_ack")

    def batch_header_swap(self, arena, count: int, offsets=None, stride: int = 0, stream=None) -> None:
        """TcpHeaderN2H (== TcpHeaderH2N, tcp-header.h:193-221) in place on the first 32 bytes of
        every image (tcpck_batch_header_swap); after VERIFY this completes ReceivePacket's
        front half (socket-manager.h:182-184)."""
        _check(self._L.tcpck_batch_header_swap(self._h, _ptr(arena), _ptr(offsets), stride, count,
                                             _stream(stream)), "tcpck_batch_header_swap")

    def batch_receive(self, arena, count: int, ok, hdr=None, stride: int = 0, length: int = 0, offsets=None,
                      lengths=None, mode: int = MODE_REF, total_bytes: int = 0, min_len: int = 0, max_len: int = 0,
                      packed: bool = False, sorted: bool = False, stream=None, kernel: int | None = None,
                      param: int = 0, probe_flags: int | None = None) -> None:
        """ReceivePacket's front half for a batch (tcpck_batch_receive): ok[k] = verdict on the
        network-order image; headers in host order in place (hdr None) or into hdr (32 B per image,
        the arena left as received).  Fixed layout (stride, length) or offsets + lengths.
        kernel/param: tcpck_batch_receive_ex (include/tcpck_tuning.h); probe_flags (probe contexts
        only): tcpck_probe_receive_ex's header pass forms (PROBE_RECEIVE_*, include/tcpck_probe.h)."""
        lay = Layout(total_bytes, min_len, max_len,
                     (LAYOUT_PACKED if packed else 0) | (LAYOUT_SORTED if sorted else 0), 0)
        args = (self._h, mode, _ptr(arena), stride, length, _ptr(offsets), _ptr(lengths), count, _ptr(ok), _ptr(hdr),
                ctypes.byref(lay))
        if probe_flags is not None:
            _check(self._L.tcpck_probe_receive_ex(*args, kernel or KERNEL_AUTO, param, probe_flags, _stream(stream)),
                   "tcpck_probe_receive_ex")
        elif kernel is None:
            _check(self._L.tcpck_batch_receive(*args, _stream(stream)), "tcpck_batch_receive")
        else:
            _check(self._L.tcpck_batch_receive_ex(*args, kernel, param, _stream(stream)), "tcpck_batch_receive_ex")

    def batch_deliver(self, arena, count: int, dst, recv, recv_bytes: int, stride: int = 0, length: int = 0,
                      offsets=None, lengths=None, stream=None) -> None:
        """Accept()'s payload append for a batch (tcpck_batch_deliver, socket-internal.h:323-334):
        recv[dst[k], dst[k] + len_k - 32) = bytes 32.. of image k for every k with dst[k] !=
        DELIVER_SKIP; every other byte of recv keeps its value.  Layout as batch_receive."""
        _check(self._L.tcpck_batch_deliver(self._h, _ptr(arena), stride, length, _ptr(offsets), _ptr(lengths), count,
                                           _ptr(dst), _ptr(recv), recv_bytes, _stream(stream)), "tcpck_batch_deliver")

    def batch_demux(self, table: "ConnTable", hdr, count: int, conn, stream=None) -> None:
        """ReceivePacket's socket lookup for a batch (tcpck_batch_demux, socket-manager.h:187-196):
        conn[k] (u32) = the id `table`, as last committed, holds for image k's key -- (dst port, src
        address, src port), or (dst port, 0, 0) for a SYN without ACK -- else CONN_NONE.  hdr: the
        dense host-order header array batch_receive writes."""
        _check(self._L.tcpck_batch_demux(self._h, table._h if table is not None else None, _ptr(hdr), count,
                                         _ptr(conn), _stream(stream)), "tcpck_batch_demux")

    def batch_reply(self, verdict, ack, tmpl, n_conns: int, count: int, replies, reply_cap: int, total, scratch,
                    conn=None, src=None, mode: int = MODE_REF, stream=None) -> None:
        """The planners' verdicts -> the dense, checksummed, network-order ACK / RST ring
        (tcpck_batch_reply): device arrays verdict u8[count], ack u32[count], conn u32[count] or None
        (every image connection 0), tmpl 32 B per connection; reply j at replies + 32 j for j <
        reply_cap, src[j] (u32, or None) the image it answers, total (one u64) the number of replying
        images; scratch: reply_scratch_bytes(count) bytes of device memory."""
        _check(self._L.tcpck_batch_reply(self._h, mode, _ptr(verdict), _ptr(ack), _ptr(conn), _ptr(tmpl), n_conns, count,
                                         _ptr(replies), reply_cap, _ptr(src), _ptr(total), _ptr(scratch),
                                         _stream(stream)), "tcpck_batch_reply")

    def batch_resend(self, arena, arena_bytes: int, snd, n_conns: int, count: int, total, scratch, stride: int = 0,
                     length: int = 0, offsets=None, lengths=None, conn=None, keep=None, out_offsets=None,
                     out_lengths=None, out_conn=None, src=None, out_cap: int = 0, rule: int = RESEND_REF,
                     mode: int = MODE_REF, stream=None) -> None:
        """The reference's resend event over a whole send queue (tcpck_batch_resend; ResendPredicate,
        socket-internal.h:363-390): device arrays; image k at k * stride (`length` bytes) or at offsets[k]
        (lengths[k] bytes), its connection conn[k] (None: 0), snd 16 B of (snd_una, rcv_nxt, flags,
        reserved) per connection.  Kept images get ACK number := htonl(rcv_nxt) and the checksum updated in
        place; keep[k] (u8), the survivors' out_offsets (u64) / out_lengths / out_conn / src (u32) dense
        and in queue order for j < out_cap (each may be None), total (one u64) the number kept; scratch:
        resend_scratch_bytes(count) bytes of device memory."""
        _check(self._L.tcpck_batch_resend(self._h, mode, rule, _ptr(arena), arena_bytes, stride, length, _ptr(offsets),
                                          _ptr(lengths), _ptr(conn), _ptr(snd), n_conns, count, _ptr(keep),
                                          _ptr(out_offsets), _ptr(out_lengths), _ptr(out_conn), _ptr(src), out_cap,
                                          _ptr(total), _ptr(scratch), _stream(stream)), "tcpck_batch_resend")

    def batch_segment(self, payload, payload_bytes: int, seg: int, hdr, seq0: int, images, stride: int,
                      out=None, mode: int = MODE_REF, param: int | None = None, stream=None) -> int:
        """Send stream -> checksummed images (tcpck_batch_segment): image k at k * stride
        = hdr with TcpLength/seq of segment k + payload[k seg, ...), checksum filled.
        hdr: 32 bytes (network order).  Returns the number of images."""
        h = _as_u8(hdr)
        if h.size != 32:
            raise ValueError("hdr must be 32 bytes")
        args = (self._h, mode, _ptr(payload), payload_bytes, seg, h.ctypes.data, seq0 & 0xFFFFFFFF, _ptr(images),
                stride, _ptr(out))
        if param is None:
            _check(self._L.tcpck_batch_segment(*args, _stream(stream)), "tcpck_batch_segment")
        else:
            _check(self._L.tcpck_batch_segment_ex(*args, param, _stream(stream)), "tcpck_batch_segment_ex")
        return (payload_bytes + seg - 1) // seg

    # explicit kernel choice (include/tcpck_tuning.h)
    def batch_fixed_ex(self, op: int, arena, stride: int, length: int, count: int, out, kernel: int,
                       param: int = 0, mode: int = MODE_REF, stream=None) -> None:
        _check(self._L.tcpck_batch_fixed_ex(self._h, op, mode, _ptr(arena), stride, length, count,
                                          _ptr(out), kernel, param, _stream(stream)), "tcpck_batch_fixed_ex")

    def batch_var_ex(self, op: int, arena, offsets, lengths, count: int, out, kernel: int,
                     param: int = 0, mode: int = MODE_REF, total_bytes: int = 0, min_len: int = 0,
                     max_len: int = 0, packed: bool = False, sorted: bool = False, stream=None) -> None:
        lay = Layout(total_bytes, min_len, max_len,
                     (LAYOUT_PACKED if packed else 0) | (LAYOUT_SORTED if sorted else 0), 0)
        _check(self._L.tcpck_batch_var_ex(self._h, op, mode, _ptr(arena), _ptr(offsets), _ptr(lengths),
                                        count, _ptr(out), ctypes.byref(lay), kernel, param,
                                        _stream(stream)), "tcpck_batch_var_ex")

    # host-memory batches (end to end, PCIe included)
    def host_batch_fixed(self, op: int, arena, stride: int, length: int, count: int, out,
                         mode: int = MODE_REF) -> None:
        _check(self._L.tcpck_host_batch_fixed(self._h, op, mode, _ptr(arena), stride, length, count,
                                            _ptr(out)), "tcpck_host_batch_fixed")

    def host_batch_var(self, op: int, arena, offsets, lengths, count: int, out,
                       mode: int = MODE_REF) -> None:
        _check(self._L.tcpck_host_batch_var(self._h, op, mode, _ptr(arena), _ptr(offsets),
                                          _ptr(lengths), count, _ptr(out)), "tcpck_host_batch_var")

    def diag_stream(self, variant: int, buf, nbytes: int, out, stream=None) -> None:
        """Timing-only streaming micro-kernel (include/tcpck_tuning.h)."""
        _check(self._L.tcpck_diag_stream(self._h, variant, _ptr(buf), nbytes, _ptr(out), _stream(stream)),
               "tcpck_diag_stream")

    def set_debug(self, buf) -> None:
        """Per-wave {start, end, hw_id, xcc_id} stamp buffer for timing builds (None = off)."""
        _check(self._L.tcpck_ctx_set_debug(self._h, _ptr(buf)), "tcpck_ctx_set_debug")

    def scratch_state(self) -> tuple[int, int]:
        """(slots allocated, bit mask of slots used) of the out-less FILL results
        scratch (libtcpck_probe.so only, tcpck_probe.h)."""
        a, m = ctypes.c_int(), ctypes.c_int()
        _check(self._L.tcpck_probe_scratch_state(self._h, ctypes.byref(a), ctypes.byref(m)),
               "tcpck_probe_scratch_state")
        return a.value, m.value

    def scratch_fail(self, n: int) -> int:
        """Refuse the next n scratch allocations (fault injection, libtcpck_probe.so only);
        returns the refusals so far."""
        r = ctypes.c_uint64()
        _check(self._L.tcpck_probe_scratch_fail(self._h, n, ctypes.byref(r)), "tcpck_probe_scratch_fail")
        return r.value

    def set_fill_pipe(self, k: int, prio: int = 0) -> None:
        """The pipelined FILL under AUTO in this context: k chunks (0/1 serial, -1 AUTO's rule), the
        field passes on a context stream of priority prio (libtcpck_probe.so only, tcpck_probe.h)."""
        _check(self._L.tcpck_probe_set_fill_pipe(self._h, k, prio), "tcpck_probe_set_fill_pipe")

    def set_deliver_grid(self, run: int = 0, max_blocks: int = 0):
        """batch_deliver's launch grid in this context (libtcpck_probe.so only, tcpck_probe.h): run > 0
        images per block, max_blocks > 0 the cap on the grid, 0 the launcher's own rule.  Returns
        (blocks, per_block, rem) of the context's last deliver launch."""
        b, q, r = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.tcpck_probe_set_deliver_grid(self._h, run, max_blocks, ctypes.byref(b), ctypes.byref(q),
                                                    ctypes.byref(r)), "tcpck_probe_set_deliver_grid")
        self._deliver_grid = (run, max_blocks)
        return b.value, q.value, r.value

    def deliver_split(self):
        """(blocks, per_block, rem) of the context's last deliver launch; the grid setting stays."""
        return self.set_deliver_grid(*getattr(self, "_deliver_grid", (0, 0)))

    def set_chunk_bytes(self, n: int) -> None:
        _check(self._L.tcpck_ctx_set_chunk_bytes(self._h, n), "tcpck_ctx_set_chunk_bytes")


def _ctx_array(ctxs):
    if len({c.probe for c in ctxs}) > 1:
        raise ValueError("contexts of libtcpck.so and libtcpck_probe.so cannot be mixed")
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def host_batch_fixed_multi(ctxs, op: int, arena, stride: int, length: int, count: int, out,
                           mode: int = MODE_REF) -> None:
    """tcpck_host_batch_fixed over several contexts (one per GPU): contiguous equal shards, one host thread each."""
    p, keep = _ctx_array(ctxs)
    _check(ctxs[0]._L.tcpck_host_batch_fixed_multi(p, len(ctxs), op, mode, _ptr(arena), stride, length, count, _ptr(out)),
           "tcpck_host_batch_fixed_multi")
    del keep


def host_batch_var_multi(ctxs, op: int, arena, offsets, lengths, count: int, out, mode: int = MODE_REF) -> None:
    """tcpck_host_batch_var over several contexts: contiguous shards balanced by bytes."""
    p, keep = _ctx_array(ctxs)
    _check(ctxs[0]._L.tcpck_host_batch_var_multi(p, len(ctxs), op, mode, _ptr(arena), _ptr(offsets), _ptr(lengths), count,
                                            _ptr(out)), "tcpck_host_batch_var_multi")
    del keep
