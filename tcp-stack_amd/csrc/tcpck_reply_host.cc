// tcpck_reply_host.cc -- tcpck_build_replies (include/tcpck.h): the batched
// reply builder on host arrays, the twin of tcpck_batch_reply (tcpck_reply.hip)
// and its CPU fallback.  Plain host C++ (no HIP), reentrant, no allocation.
//
// Per replying image, what the reference sends (SocketInternal::SendAck,
// include/socket-internal.h:293-299, through SocketManager::SendPacket,
// src/socket-manager.cc:6-12; the RST of a datagram of no socket,
// include/socket-manager.h:201-207): the 32 header bytes in network order, the
// checksum stored by tcpck_fill16 itself.
#include <cstring>

#include "tcpck_reply.h"

namespace {

void put_be32(uint8_t *p, uint32_t v) {  // htonl
  p[0] = static_cast<uint8_t>(v >> 24);
  p[1] = static_cast<uint8_t>(v >> 16);
  p[2] = static_cast<uint8_t>(v >> 8);
  p[3] = static_cast<uint8_t>(v);
}

}  // namespace

extern "C" int tcpck_build_replies(int mode, const uint8_t *h_verdict, const uint32_t *h_ack, const uint32_t *h_conn,
                                   const void *h_tmpl, uint32_t n_conns, uint64_t count, void *h_replies,
                                   uint64_t reply_cap, uint32_t *h_src, uint64_t *n_replies) {
  const int rc = tcpck::reply::check(mode, h_verdict, h_ack, h_conn, h_tmpl, n_conns, count, h_replies, h_src, n_replies);
  if (rc != TCPCK_OK) return rc;
  const uint8_t *tmpl = static_cast<const uint8_t *>(h_tmpl);
  uint8_t *out = static_cast<uint8_t *>(h_replies);
  uint64_t j = 0;
  for (uint64_t k = 0; k < count; ++k) {
    const uint32_t v = h_verdict[k];
    uint8_t image[TCPCK_REPLY_BYTES];
    if (v & TCPCK_RCV_RST) {
      std::memset(image, 0, sizeof image);
      put_be32(image + 16, h_ack[k]);  // RstHeader: seq = the image's acknowledgement number
      image[25] = 0x20;
    } else if (v & TCPCK_RCV_SEND_ACK) {
      const uint32_t c = h_conn ? h_conn[k] : 0;
      if (c >= n_conns) continue;  // TCPCK_CONN_NONE included: no template is read outside [0, n_conns)
      std::memcpy(image, tmpl + 32ull * c, sizeof image);
      put_be32(image + 20, h_ack[k]);  // AckHeader: AcknowledgementNumber
      image[25] |= 0x08;
    } else {
      continue;
    }
    if (j < reply_cap) {
      tcpck_fill16(image, sizeof image, mode, nullptr);  // Checksum() = 0; Checksum() = CalculateChecksum(*p)
      std::memcpy(out + 32 * j, image, sizeof image);
      if (h_src) h_src[j] = static_cast<uint32_t>(k);
    }
    ++j;
  }
  if (n_replies) *n_replies = j;
  return TCPCK_OK;
}
