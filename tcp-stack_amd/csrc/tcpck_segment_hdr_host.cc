// tcpck_segment_hdr_host.cc -- tcpck_plan_cuts and tcpck_segment_headers
// (include/tcpck.h): the send ring's planner, and zero-copy segmentation on
// host arrays, the twin of tcpck_batch_segment_headers (tcpck_segment_hdr.hip)
// and its CPU fallback.  Plain host C++ (no HIP), reentrant, no allocation.
//
// Per segment, what the reference puts in front of the payload
// (TcpSendingBuffer::GetAsTcpPacket, include/tcp-buffer.h:82-98; Estab's
// kSend, src/state.cc:167-184; TcpHeaderH2N; the checksum of
// include/socket-manager.h:259-260 over header and payload) -- the payload
// itself stays in the send stream, where TcpSendingBuffer::Ack
// (include/tcp-buffer.h:51-68) keeps it until it is acknowledged.
#include <cstring>

#include "tcpck_segment_hdr.h"

namespace seghdr = tcpck::seghdr;

extern "C" int tcpck_plan_cuts(tcpck_send_cut *h_cuts, uint32_t n_cuts, uint32_t seg, uint64_t payload_bytes,
                               uint32_t n_tmpl, uint64_t *n_seg) {
  if (!n_seg || (n_cuts && !h_cuts) || !seghdr::valid_seg(seg) || (payload_bytes & 1)) return TCPCK_EINVAL;
  uint64_t total = 0;
  for (uint32_t c = 0; c < n_cuts; ++c) {
    if (!seghdr::in_bounds(h_cuts[c].offset, h_cuts[c].bytes, h_cuts[c].tmpl, payload_bytes, n_tmpl)) return TCPCK_EINVAL;
    total += seghdr::segments_of(h_cuts[c].bytes, seg);
    if (total > seghdr::kMaxSegments) return TCPCK_EINVAL;
  }
  uint32_t first = 0;
  for (uint32_t c = 0; c < n_cuts; ++c) {
    h_cuts[c].first = first;
    first += seghdr::segments_of(h_cuts[c].bytes, seg);
  }
  *n_seg = total;
  return TCPCK_OK;
}

extern "C" int tcpck_segment_headers(int mode, const void *h_payload, uint64_t payload_bytes, uint32_t seg,
                                     const tcpck_send_cut *h_cuts, uint32_t n_cuts, const void *h_tmpl, uint32_t n_tmpl,
                                     uint64_t n_seg, void *h_hdr, uint64_t *h_pay_off, uint32_t *h_pay_len,
                                     uint16_t *h_out) {
  const int rc = seghdr::check(mode, h_payload, payload_bytes, seg, h_cuts, n_cuts, h_tmpl, n_tmpl, n_seg, h_hdr,
                               h_pay_off, h_pay_len, h_out);
  if (rc != TCPCK_OK || n_seg == 0) return rc;
  const uint8_t *payload = static_cast<const uint8_t *>(h_payload);
  uint8_t *hdr = static_cast<uint8_t *>(h_hdr);
  // a ring index no sound cut claims: zero header, offset, length and checksum
  std::memset(hdr, 0, 32 * n_seg);
  if (h_pay_off) std::memset(h_pay_off, 0, sizeof(uint64_t) * n_seg);
  if (h_pay_len) std::memset(h_pay_len, 0, sizeof(uint32_t) * n_seg);
  if (h_out) std::memset(h_out, 0, sizeof(uint16_t) * n_seg);
  for (uint32_t c = 0; c < n_cuts; ++c) {
    if (!seghdr::sound(h_cuts, n_cuts, c, seg, payload_bytes, n_tmpl, n_seg)) continue;
    const tcpck_send_cut &cut = h_cuts[c];
    const uint32_t n = seghdr::segments_of(cut.bytes, seg);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t at = i * seg;  // < bytes
      const uint32_t len = cut.bytes - at < seg ? cut.bytes - at : seg;
      const uint32_t seq = cut.seq0 + at;  // wraps as snd_nxt does
      uint8_t image[32];
      std::memcpy(image, static_cast<const uint8_t *>(h_tmpl) + 32ull * cut.tmpl, 32);
      image[10] = static_cast<uint8_t>(len >> 8);  // TcpLength, htons
      image[11] = static_cast<uint8_t>(len);
      image[16] = static_cast<uint8_t>(seq >> 24);  // SequenceNumber, htonl
      image[17] = static_cast<uint8_t>(seq >> 16);
      image[18] = static_cast<uint8_t>(seq >> 8);
      image[19] = static_cast<uint8_t>(seq);
      image[28] = image[29] = 0;  // Checksum() = 0 (socket-manager.h:259)
      // the image's word sum is the header's plus the payload's: each call
      // returns ~sum (REF: mod 2^16; RFC 1071: folded, zero only for all-zero words)
      uint16_t ch = 0, cp = 0;
      tcpck_checksum16(image, 32, mode, &ch);
      tcpck_checksum16(payload + cut.offset + at, len, mode, &cp);
      uint32_t sum = static_cast<uint32_t>(static_cast<uint16_t>(~ch)) + static_cast<uint16_t>(~cp);
      if (mode == TCPCK_MODE_RFC1071) sum = (sum & 0xFFFFu) + (sum >> 16);
      const uint16_t csum = static_cast<uint16_t>(~sum);
      std::memcpy(image + 28, &csum, 2);
      const uint64_t g = static_cast<uint64_t>(cut.first) + i;
      std::memcpy(hdr + 32 * g, image, 32);
      if (h_pay_off) h_pay_off[g] = cut.offset + at;
      if (h_pay_len) h_pay_len[g] = len;
      if (h_out) h_out[g] = csum;
    }
  }
  return TCPCK_OK;
}
