// tcpck_deliver_plan.cc -- tcpck_plan_deliver (include/tcpck.h): which images
// of an arrival sequence an established connection accepts, and where their
// payloads go in the receive stream; tcpck_plan_deliver_multi: the same walk
// over a ring that mixes many connections (h_conn[k] from tcpck_batch_demux),
// through the same per-image step.  Control plane: a serial chain over 32 B
// of header per image, so it runs on the host over the dense header array
// tcpck_batch_receive writes; the per-byte copy is tcpck_batch_deliver's kernel
// (tcpck_deliver.hip).
//
// Reference (filixi/TCP-stack), per arriving packet:
//   SocketInternal::RecvPacket              include/socket-internal.h:161-171
//     !check_sum_validate: state_.InvalideCheckSum() -- Discard, SendAck(snd_nxt,
//     rcv_nxt, wnd) (include/state.h:268-275); else state_(header)
//   Estab::operator()(const TcpHeader &, b) src/state.cc:195-223
//     IsAck && ack <= snd_nxt && seq == rcv_nxt: snd_una = max(ack, snd_una),
//     rcv_nxt = seq + TcpLength, rcv_wnd = window; Accept, RecvAck, SendAck if
//     TcpLength; IsFin && ...: leaves Estab (CloseWait); else Discard
//   SocketInternal::Accept                  include/socket-internal.h:323-334
//     TcpLength > 0: recv_buffer_ gets packet->begin()..end()
//
// Plain host C++ (no HIP), reentrant: all state is the caller's.
#include <cstdint>
#include <cstring>

#include "tcpck.h"

namespace {

// the reference's flag bits in header byte 25 (tcp-header.h:122-162: bits
// 106-111 of the 20-byte TCP part)
constexpr uint8_t kAck = 0x08, kSyn = 0x40, kFin = 0x80;

template <typename T>
T field(const uint8_t *h, int at) {
  T v;
  std::memcpy(&v, h + at, sizeof(T));
  return v;
}

// One image of the walk, RecvPacket then Estab: false where the walk stops
// before it (the FIN in sequence that leaves Estab, a payload that does not
// fit in recv_bytes) with `s` and `reply` untouched; else the image's verdict,
// reply ack and destination (relative to the receive stream, or SKIP), `s`
// advanced.  Both planners below run exactly this.
inline bool plan_step(const uint8_t *h, bool ok, uint32_t length, tcpck_rcv_state &s, uint64_t recv_bytes,
                      uint64_t &dst, uint8_t &verdict, uint32_t &reply) {
  dst = TCPCK_DELIVER_SKIP;
  verdict = 0;
  if (!ok) {  // InvalideCheckSum: Discard, SendAck(snd_nxt, rcv_nxt, wnd)
    verdict = TCPCK_RCV_BAD_SUM | TCPCK_RCV_SEND_ACK;
    reply = s.rcv_nxt;
    return true;
  }
  const uint16_t tcp_length = field<uint16_t>(h, 10);
  const uint32_t seq = field<uint32_t>(h, 16), ack = field<uint32_t>(h, 20);
  const uint8_t flags = h[25];
  const bool in_order = ack <= s.snd_nxt && seq == s.rcv_nxt;
  if (in_order && (flags & (kAck | kSyn | kFin)) == (kAck | kFin)) return false;  // IsFin: leaves Estab
  if (in_order && (flags & (kAck | kSyn | kFin)) == kAck) {                       // IsAck
    const uint32_t payload = length - TCPCK_HEADER_BYTES;
    const bool append = tcp_length > 0 && payload > 0;
    if (append && payload > recv_bytes - s.delivered) return false;  // the receive stream is full
    s.snd_una = ack > s.snd_una ? ack : s.snd_una;
    s.rcv_nxt = seq + tcp_length;
    s.rcv_wnd = field<uint16_t>(h, 26);
    verdict = TCPCK_RCV_ACCEPT;
    if (tcp_length > 0) verdict |= TCPCK_RCV_SEND_ACK;
    if (append) {
      verdict |= TCPCK_RCV_PAYLOAD;
      dst = s.delivered;
      s.delivered += payload;
    }
  }
  reply = s.rcv_nxt;
  return true;
}

bool bad_lengths(const uint32_t *h_lengths, uint32_t len, uint64_t count) {
  if (!h_lengths) return count && ((len & 1) || len < TCPCK_HEADER_BYTES);
  for (uint64_t k = 0; k < count; ++k)
    if ((h_lengths[k] & 1) || h_lengths[k] < TCPCK_HEADER_BYTES) return true;
  return false;
}

}  // namespace

extern "C" int tcpck_plan_deliver(const void *h_hdr, const uint8_t *h_ok, const uint32_t *h_lengths, uint32_t len,
                                  uint64_t count, tcpck_rcv_state *st, uint64_t recv_bytes, uint64_t *h_dst,
                                  uint8_t *h_verdict, uint32_t *h_ack, uint64_t *consumed) {
  if (!st || !consumed) return TCPCK_EINVAL;
  if (count && (!h_hdr || !h_ok || !h_dst || !h_verdict || !h_ack)) return TCPCK_EINVAL;
  if (bad_lengths(h_lengths, len, count)) return TCPCK_EINVAL;
  if (st->delivered > recv_bytes) return TCPCK_EINVAL;

  const uint8_t *hdr = static_cast<const uint8_t *>(h_hdr);
  tcpck_rcv_state s = *st;
  uint64_t k = 0;
  for (; k < count; ++k)
    if (!plan_step(hdr + TCPCK_HEADER_BYTES * k, h_ok[k] != 0, h_lengths ? h_lengths[k] : len, s, recv_bytes, h_dst[k],
                   h_verdict[k], h_ack[k]))
      break;
  *consumed = k;
  for (; k < count; ++k) {
    h_dst[k] = TCPCK_DELIVER_SKIP;
    h_verdict[k] = 0;
    h_ack[k] = s.rcv_nxt;
  }
  *st = s;
  return TCPCK_OK;
}

// The same walk over a ring that mixes connections (include/tcpck.h): image k
// steps the state of conns[h_conn[k]]; a connection that stops does so alone.
// Images of no socket follow SocketManager::ReceivePacket's else branch
// (include/socket-manager.h:197-207): ok -> RST with seq = the packet's ack
// number (RstHeader, include/socket-internal.h:43-50), else nothing.
extern "C" int tcpck_plan_deliver_multi(const void *h_hdr, const uint8_t *h_ok, const uint32_t *h_conn,
                                        const uint32_t *h_lengths, uint32_t len, uint64_t count,
                                        tcpck_conn_state *conns, uint32_t n_conns, uint64_t *h_dst,
                                        uint8_t *h_verdict, uint32_t *h_ack) {
  if (count && (!h_hdr || !h_ok || !h_conn || !h_dst || !h_verdict || !h_ack)) return TCPCK_EINVAL;
  if (n_conns && !conns) return TCPCK_EINVAL;
  if (bad_lengths(h_lengths, len, count)) return TCPCK_EINVAL;
  for (uint64_t k = 0; k < count; ++k)
    if (h_conn[k] != TCPCK_CONN_NONE && h_conn[k] >= n_conns) return TCPCK_EINVAL;
  for (uint32_t c = 0; c < n_conns; ++c) {
    const tcpck_conn_state &cs = conns[c];
    if ((cs.recv_base & 1) || cs.recv_bytes > UINT64_MAX - cs.recv_base || cs.rcv.delivered > cs.recv_bytes)
      return TCPCK_EINVAL;
  }

  for (uint32_t c = 0; c < n_conns; ++c) conns[c].stopped_at = TCPCK_NOT_STOPPED;
  const uint8_t *hdr = static_cast<const uint8_t *>(h_hdr);
  bool host_seen = false;  // an earlier image went to the host path: the table may be behind
  for (uint64_t k = 0; k < count; ++k) {
    const uint8_t *h = hdr + TCPCK_HEADER_BYTES * k;
    const uint32_t c = h_conn[k];
    h_dst[k] = TCPCK_DELIVER_SKIP;
    h_verdict[k] = 0;
    if (c == TCPCK_CONN_NONE) {
      h_ack[k] = 0;
      if (!h_ok[k]) continue;
      if (host_seen) {
        h_verdict[k] = TCPCK_RCV_HOST;
      } else {
        h_verdict[k] = TCPCK_RCV_RST;
        h_ack[k] = field<uint32_t>(h, 20);
      }
      continue;
    }
    tcpck_conn_state &cs = conns[c];
    if (cs.flags & TCPCK_CONN_HOST) {
      h_verdict[k] = TCPCK_RCV_HOST;
      h_ack[k] = cs.rcv.rcv_nxt;
      host_seen = true;
      continue;
    }
    if (cs.stopped_at == TCPCK_NOT_STOPPED) {
      uint64_t dst;
      if (plan_step(h, h_ok[k] != 0, h_lengths ? h_lengths[k] : len, cs.rcv, cs.recv_bytes, dst, h_verdict[k],
                    h_ack[k])) {
        if (dst != TCPCK_DELIVER_SKIP) h_dst[k] = cs.recv_base + dst;
        continue;
      }
      cs.stopped_at = k;
      h_verdict[k] = 0;
    }
    h_ack[k] = cs.rcv.rcv_nxt;
  }
  return TCPCK_OK;
}
