// tcpck_reply.h -- what the batched reply builder's device side (tcpck_reply.hip)
// and its host twin (tcpck_reply_host.cc) share: the one block-size constant
// behind tcpck_reply_scratch_bytes and the launcher, and the argument checks of
// tcpck_batch_reply / tcpck_build_replies (include/tcpck.h).  Plain C++, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

#include "tcpck.h"

namespace tcpck {
namespace reply {

constexpr uint64_t kMaxCount = 1ull << 31;    // images per call: every image and reply index fits in a u32
constexpr uint32_t kImagesPerBlock = 1024;    // images per block of the count and emit passes

inline uint64_t blocks_for(uint64_t count) { return (count + kImagesPerBlock - 1) / kImagesPerBlock; }

// one u32 per block (its total, then its offset), rounded up to whole 16-B units; never 0
inline size_t scratch_bytes(uint64_t count) {
  const uint64_t bytes = (4 * blocks_for(count) + 15) & ~uint64_t{15};
  return static_cast<size_t>(bytes ? bytes : 16);
}

inline bool misaligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }

// The clauses both entry points share (the device one adds ctx and d_scratch).
inline int check(int mode, const uint8_t *verdict, const uint32_t *ack, const uint32_t *conn, const void *tmpl,
                 uint32_t n_conns, uint64_t count, const void *replies, const uint32_t *src, const uint64_t *total) {
  if (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071) return TCPCK_EINVAL;
  if (count > kMaxCount) return TCPCK_EINVAL;
  if (count > 0 && (!verdict || !ack || !replies || !total)) return TCPCK_EINVAL;
  if (n_conns > 0 && !tmpl) return TCPCK_EINVAL;
  if (misaligned(ack, 4) || misaligned(conn, 4) || misaligned(src, 4)) return TCPCK_EINVAL;
  if (misaligned(tmpl, 16) || misaligned(replies, 16) || misaligned(total, 8)) return TCPCK_EINVAL;
  return TCPCK_OK;
}

}  // namespace reply
}  // namespace tcpck
