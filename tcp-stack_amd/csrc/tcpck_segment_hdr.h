// tcpck_segment_hdr.h -- what zero-copy segmentation's device side
// (tcpck_segment_hdr.hip) and its host twin (tcpck_segment_hdr_host.cc) share:
// the rule that says which cuts of a send ring's cut table count, and the
// argument checks of tcpck_batch_segment_headers / tcpck_segment_headers
// (include/tcpck.h).  Plain C++; the rule also compiles as device code.
#pragma once

#include <cstddef>
#include <cstdint>

#include "tcpck.h"

#if defined(__HIPCC__)
#define TCPCK_SEGHDR_FN __host__ __device__ __forceinline__
#else
#define TCPCK_SEGHDR_FN inline
#endif

namespace tcpck {
namespace seghdr {

constexpr uint64_t kMaxSegments = 1ull << 31;  // ring indices and first + segments fit in a u32

TCPCK_SEGHDR_FN bool valid_seg(uint32_t seg) { return seg >= 16 && seg <= 65532 && !(seg & 3); }

// ceil(bytes / seg) without leaving 32 bits
TCPCK_SEGHDR_FN uint32_t segments_of(uint32_t bytes, uint32_t seg) { return bytes / seg + (bytes % seg ? 1u : 0u); }

// The clauses of tcpck_plan_cuts a cut can break on its own.
TCPCK_SEGHDR_FN bool in_bounds(uint64_t offset, uint32_t bytes, uint32_t tmpl, uint64_t payload_bytes, uint32_t n_tmpl) {
  return !(offset & 3) && !(bytes & 1) && offset <= payload_bytes && bytes <= payload_bytes - offset && tmpl < n_tmpl;
}

// A cut counts -- it is *sound* -- when it is in bounds, its segments lie in
// [0, n_seg), and a neighbour confirms its `first`: the cut before it ends
// where it starts (cut 0: it starts at 0), or it ends where the cut after it
// starts (the last cut: at n_seg).  A planned table is sound throughout; one
// cut damaged in any field takes only its own segments out, since each of its
// neighbours is still confirmed from its other side.  Local to three entries,
// so every wave decides it alone and the host twin decides the same.
TCPCK_SEGHDR_FN bool sound(const tcpck_send_cut *cuts, uint32_t n_cuts, uint32_t c, uint32_t seg, uint64_t payload_bytes,
                           uint32_t n_tmpl, uint64_t n_seg) {
  const uint64_t offset = cuts[c].offset;
  const uint32_t bytes = cuts[c].bytes, first = cuts[c].first;
  if (!in_bounds(offset, bytes, cuts[c].tmpl, payload_bytes, n_tmpl)) return false;
  const uint64_t end = static_cast<uint64_t>(first) + segments_of(bytes, seg);
  if (end > n_seg) return false;
  const bool left = c == 0 ? first == 0
                           : static_cast<uint64_t>(cuts[c - 1].first) + segments_of(cuts[c - 1].bytes, seg) == first;
  if (left) return true;
  return c + 1 == n_cuts ? end == n_seg : end == cuts[c + 1].first;
}

inline bool misaligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }

// The clauses both entry points share (the device one adds ctx).
inline int check(int mode, const void *payload, uint64_t payload_bytes, uint32_t seg, const tcpck_send_cut *cuts,
                 uint32_t n_cuts, const void *tmpl, uint32_t n_tmpl, uint64_t n_seg, const void *hdr,
                 const uint64_t *pay_off, const uint32_t *pay_len, const uint16_t *out) {
  if (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071) return TCPCK_EINVAL;
  if (!valid_seg(seg) || (payload_bytes & 1) || n_seg > kMaxSegments) return TCPCK_EINVAL;
  if (misaligned(payload, 4) || misaligned(hdr, 16) || misaligned(tmpl, 16) || misaligned(cuts, 8)) return TCPCK_EINVAL;
  if (misaligned(pay_off, 8) || misaligned(pay_len, 4) || misaligned(out, 2)) return TCPCK_EINVAL;
  if (n_seg == 0) return TCPCK_OK;
  if (!hdr || (payload_bytes && !payload) || (n_cuts && !cuts) || (n_tmpl && !tmpl)) return TCPCK_EINVAL;
  return TCPCK_OK;
}

}  // namespace seghdr
}  // namespace tcpck
