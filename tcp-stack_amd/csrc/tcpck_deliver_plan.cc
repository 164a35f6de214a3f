// tcpck_deliver_plan.cc -- tcpck_plan_deliver (include/tcpck.h): which images
// of an arrival sequence an established connection accepts, and where their
// payloads go in the receive stream.  Control plane: a serial chain over 32 B
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

}  // namespace

extern "C" int tcpck_plan_deliver(const void *h_hdr, const uint8_t *h_ok, const uint32_t *h_lengths, uint32_t len,
                                  uint64_t count, tcpck_rcv_state *st, uint64_t recv_bytes, uint64_t *h_dst,
                                  uint8_t *h_verdict, uint32_t *h_ack, uint64_t *consumed) {
  if (!st || !consumed) return TCPCK_EINVAL;
  if (count && (!h_hdr || !h_ok || !h_dst || !h_verdict || !h_ack)) return TCPCK_EINVAL;
  if (!h_lengths && count && ((len & 1) || len < TCPCK_HEADER_BYTES)) return TCPCK_EINVAL;
  if (h_lengths)
    for (uint64_t k = 0; k < count; ++k)
      if ((h_lengths[k] & 1) || h_lengths[k] < TCPCK_HEADER_BYTES) return TCPCK_EINVAL;
  if (st->delivered > recv_bytes) return TCPCK_EINVAL;

  const uint8_t *hdr = static_cast<const uint8_t *>(h_hdr);
  tcpck_rcv_state s = *st;
  uint64_t k = 0;
  for (; k < count; ++k) {
    const uint8_t *h = hdr + TCPCK_HEADER_BYTES * k;
    h_dst[k] = TCPCK_DELIVER_SKIP;
    h_verdict[k] = 0;
    if (!h_ok[k]) {  // InvalideCheckSum: Discard, SendAck(snd_nxt, rcv_nxt, wnd)
      h_verdict[k] = TCPCK_RCV_BAD_SUM | TCPCK_RCV_SEND_ACK;
      h_ack[k] = s.rcv_nxt;
      continue;
    }
    const uint16_t tcp_length = field<uint16_t>(h, 10);
    const uint32_t seq = field<uint32_t>(h, 16), ack = field<uint32_t>(h, 20);
    const uint8_t flags = h[25];
    const bool in_order = ack <= s.snd_nxt && seq == s.rcv_nxt;
    if (in_order && (flags & (kAck | kSyn | kFin)) == (kAck | kFin)) break;  // IsFin: leaves Estab
    if (in_order && (flags & (kAck | kSyn | kFin)) == kAck) {                // IsAck
      const uint32_t payload = (h_lengths ? h_lengths[k] : len) - TCPCK_HEADER_BYTES;
      const bool append = tcp_length > 0 && payload > 0;
      if (append && payload > recv_bytes - s.delivered) break;  // the receive stream is full
      s.snd_una = ack > s.snd_una ? ack : s.snd_una;
      s.rcv_nxt = seq + tcp_length;
      s.rcv_wnd = field<uint16_t>(h, 26);
      uint8_t v = TCPCK_RCV_ACCEPT;
      if (tcp_length > 0) v |= TCPCK_RCV_SEND_ACK;
      if (append) {
        v |= TCPCK_RCV_PAYLOAD;
        h_dst[k] = s.delivered;
        s.delivered += payload;
      }
      h_verdict[k] = v;
    }
    h_ack[k] = s.rcv_nxt;
  }
  *consumed = k;
  for (; k < count; ++k) {
    h_dst[k] = TCPCK_DELIVER_SKIP;
    h_verdict[k] = 0;
    h_ack[k] = s.rcv_nxt;
  }
  *st = s;
  return TCPCK_OK;
}
