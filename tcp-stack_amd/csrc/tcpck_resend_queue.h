// tcpck_resend_queue.h -- what the batched resend pass's device side
// (tcpck_resend_queue.hip) and its host twin (tcpck_resend_queue_host.cc) share:
// the scratch layout behind tcpck_resend_scratch_bytes and the launcher, the
// header offsets the rule reads, and the argument checks of tcpck_batch_resend /
// tcpck_resend_images (include/tcpck.h).  Plain C++, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

#include "tcpck.h"
#include "tcpck_reply.h"

namespace tcpck {
namespace resend {

constexpr uint64_t kMaxCount = reply::kMaxCount;  // images per call: every image and survivor index fits in a u32
constexpr uint32_t kMinImage = 32;                // a whole header

// The rule's header fields, as u16 word indices of the image (offsets are even):
constexpr uint32_t kWordTcpLength = 5;            // bytes 10-11, big-endian
constexpr uint32_t kWordSeq = 8;                  // bytes 16-19, big-endian: words 8, 9
constexpr uint32_t kWordAck = 10;                 // bytes 20-23: words 10, 11
constexpr uint32_t kWordFlags = 12;               // byte 25 = the word's high byte
constexpr uint32_t kWordChecksum = 14;            // bytes 28-29
constexpr uint32_t kSynFin = 0x40u | 0x80u;       // byte 25: SYN 0x40, FIN 0x80

// The scratch: one u32 per block of the mark / emit passes (its total, then its
// offset), rounded up to whole 16-B units, then one keep byte per image, rounded
// up likewise.  Never 0.
inline uint64_t totals_bytes(uint64_t count) { return (4 * reply::blocks_for(count) + 15) & ~uint64_t{15}; }
inline size_t scratch_bytes(uint64_t count) {
  const uint64_t bytes = totals_bytes(count) + ((count + 15) & ~uint64_t{15});
  return static_cast<size_t>(bytes ? bytes : 16);
}

using reply::misaligned;

// The fixed form's images that fit in the arena: image k fits iff k < fit_count
// (k * stride + len <= arena_bytes, with no product that could overflow).
inline uint64_t fit_count(uint64_t arena_bytes, uint64_t stride, uint32_t len) {
  return arena_bytes >= len ? (arena_bytes - len) / stride + 1 : 0;
}

// The clauses both entry points share (the device one adds ctx and d_scratch).
inline int check(int mode, int rule, const void *arena, uint64_t stride, uint32_t len, const uint64_t *offsets,
                 const uint32_t *lengths, const uint32_t *conn, const tcpck_snd_state *snd, uint32_t n_conns,
                 uint64_t count, const uint64_t *out_offsets, const uint32_t *out_lengths, const uint32_t *out_conn,
                 const uint32_t *src, const uint64_t *total) {
  if (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071) return TCPCK_EINVAL;
  if (rule != TCPCK_RESEND_REF && rule != TCPCK_RESEND_SERIAL) return TCPCK_EINVAL;
  if (count > kMaxCount) return TCPCK_EINVAL;
  if (count > 0 && (!arena || !total || (n_conns > 0 && !snd))) return TCPCK_EINVAL;
  if ((offsets == nullptr) != (lengths == nullptr)) return TCPCK_EINVAL;
  if (!offsets && ((stride & 1) || (len & 1) || len < kMinImage || stride < len)) return TCPCK_EINVAL;
  if (misaligned(arena, 2)) return TCPCK_EINVAL;
  if (misaligned(lengths, 4) || misaligned(conn, 4) || misaligned(out_lengths, 4) || misaligned(out_conn, 4) ||
      misaligned(src, 4))
    return TCPCK_EINVAL;
  if (misaligned(offsets, 8) || misaligned(out_offsets, 8) || misaligned(total, 8)) return TCPCK_EINVAL;
  if (misaligned(snd, 16)) return TCPCK_EINVAL;
  return TCPCK_OK;
}

}  // namespace resend
}  // namespace tcpck
