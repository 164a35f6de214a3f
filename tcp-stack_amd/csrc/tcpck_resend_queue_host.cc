// tcpck_resend_queue_host.cc -- tcpck_resend_images (include/tcpck.h): the
// batched resend pass on host memory, the twin of tcpck_batch_resend
// (tcpck_resend_queue.hip) and its CPU fallback.  Plain host C++ (no HIP),
// reentrant, no allocation.
//
// Per queued image, the reference's resend event (ResendPredicate,
// include/socket-internal.h:363-390, under InternalSendPacketWithResend,
// include/socket-manager.h:37-51): the predicate, and for a kept image the ACK
// rewrite with the checksum SendPacket (src/socket-manager.cc:9-10) would store,
// updated word by word with tcpck_update16.
#include "tcpck_resend_queue.h"

namespace {

uint32_t be32(const uint8_t *p) { return uint32_t{p[0]} << 24 | uint32_t{p[1]} << 16 | uint32_t{p[2]} << 8 | p[3]; }
uint16_t le16(const uint8_t *p) { return static_cast<uint16_t>(p[0] | p[1] << 8); }
void put_le16(uint8_t *p, uint16_t v) {
  p[0] = static_cast<uint8_t>(v);
  p[1] = static_cast<uint8_t>(v >> 8);
}

bool owed(int rule, const uint8_t *image, uint32_t snd_una) {
  const uint32_t seq = be32(image + 16);
  const uint32_t edge = (image[25] & tcpck::resend::kSynFin) ? 1u : 0u;
  if (rule == TCPCK_RESEND_REF) return snd_una < seq + edge;  // socket-internal.h:381-385, u32
  const uint32_t n = (uint32_t{image[10]} << 8 | image[11]) + edge;
  return n > 0 && static_cast<int32_t>(seq + n - snd_una) > 0;
}

}  // namespace

extern "C" int tcpck_resend_images(int mode, int rule, void *h_arena, uint64_t arena_bytes, uint64_t stride,
                                   uint32_t len, const uint64_t *h_offsets, const uint32_t *h_lengths,
                                   const uint32_t *h_conn, const tcpck_snd_state *h_snd, uint32_t n_conns,
                                   uint64_t count, uint8_t *h_keep, uint64_t *h_out_offsets, uint32_t *h_out_lengths,
                                   uint32_t *h_out_conn, uint32_t *h_src, uint64_t out_cap, uint64_t *n_kept) {
  const int rc = tcpck::resend::check(mode, rule, h_arena, stride, len, h_offsets, h_lengths, h_conn, h_snd, n_conns,
                                      count, h_out_offsets, h_out_lengths, h_out_conn, h_src, n_kept);
  if (rc != TCPCK_OK) return rc;
  uint8_t *arena = static_cast<uint8_t *>(h_arena);
  const uint64_t fit = h_offsets ? 0 : tcpck::resend::fit_count(arena_bytes, stride, len);
  uint64_t j = 0;
  for (uint64_t k = 0; k < count; ++k) {
    uint64_t off;
    uint32_t ln;
    bool ok;
    if (h_offsets) {
      off = h_offsets[k];
      ln = h_lengths[k];
      ok = !((off | ln) & 1u) && ln >= tcpck::resend::kMinImage && off <= arena_bytes && ln <= arena_bytes - off;
    } else {
      ok = k < fit;
      off = ok ? k * stride : 0;
      ln = len;
    }
    const uint32_t c = h_conn ? h_conn[k] : 0;
    // no state outside [0, n_conns) is read (TCPCK_CONN_NONE included), no byte of a dropped image written
    ok = ok && c < n_conns && !(h_snd[c].flags & TCPCK_SND_CLOSED) && owed(rule, arena + off, h_snd[c].snd_una);
    if (h_keep) h_keep[k] = ok;
    if (!ok) continue;
    uint8_t *image = arena + off;
    const uint32_t ack = h_snd[c].rcv_nxt;
    const uint8_t net[4] = {static_cast<uint8_t>(ack >> 24), static_cast<uint8_t>(ack >> 16),
                            static_cast<uint8_t>(ack >> 8), static_cast<uint8_t>(ack)};  // htonl
    uint16_t sum = le16(image + 28);
    sum = tcpck_update16(sum, le16(image + 20), le16(net), mode);
    sum = tcpck_update16(sum, le16(image + 22), le16(net + 2), mode);
    for (int i = 0; i < 4; ++i) image[20 + i] = net[i];
    put_le16(image + 28, sum);
    if (j < out_cap) {
      if (h_out_offsets) h_out_offsets[j] = off;
      if (h_out_lengths) h_out_lengths[j] = ln;
      if (h_out_conn) h_out_conn[j] = c;
      if (h_src) h_src[j] = static_cast<uint32_t>(k);
    }
    ++j;
  }
  if (n_kept) *n_kept = j;
  return TCPCK_OK;
}
