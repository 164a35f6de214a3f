// tcpck_resend_queue.hip -- the batched resend pass's device side:
// tcpck_batch_resend (include/tcpck.h) runs the reference's resend event over a
// whole send queue of many connections.
//
// Reference (filixi/TCP-stack), per queued packet:
//   SocketManager::InternalSendPacketWithResend   include/socket-manager.h:37-51
//     the timer event: predicate(packet) ? SendPacket(packet) and re-queue : drop
//   SocketInternal::ResendPredicate::operator()   include/socket-internal.h:363-390
//     dead weak_ptr -> false (:371-373); AcknowledgementNumber() = htonl(rcv_nxt)
//     (:376-377); seq = ntohl(SequenceNumber()) (:378); kClosed -> false
//     (:379-380); SYN or FIN: snd_una < seq + 1, else snd_una < seq (:381-385)
//   SocketManager::SendPacket                     src/socket-manager.cc:6-12
//     Checksum() = 0; Checksum() = CalculateChecksum(*p)
// The host twin is tcpck_resend_queue_host.cc; both follow the rule stated at
// tcpck_batch_resend in include/tcpck.h.
//
// The shape is tcpck_batch_reply's (tcpck_compact.h): a stable stream compaction
// in three launches on the caller's stream; order comes from the scan alone, no
// atomic orders anything and no block waits for another block:
//   mark   one block per kImagesPerBlock images, one image per lane: the
//          descriptor, the connection id and -- only for an id below n_conns --
//          the 16-B state block (the table stays in L2); the header's u16 words
//          (offsets are only even), the rule, and for a kept image the three
//          words of tcpck_batch_set_ack's patch (dev::update_ack) while the line
//          is in hand.  The only launch that touches the arena.  The keep byte
//          goes to the scratch (and to d_keep), the block's total to the scratch;
//   scan   ONE block turns the block totals into exclusive offsets in place and
//          stores the grand total to *d_count;
//   emit   reads the keep bytes; a kept lane's index is its block's offset + the
//          waves before it + the chunks before it + mbcnt of its chunk's ballot;
//          it stores its entry of each of the four lists at j < out_cap.
//          Consecutive kept lanes write consecutive entries.
#include <hip/hip_runtime.h>

#include "tcpck_api_internal.h"
#include "tcpck_compact.h"
#include "tcpck_device.h"
#include "tcpck_resend_queue.h"

namespace tcpck {

namespace {

using compact::kChunks;
using dev::u32x4;

struct MarkArgs {
  ImageSpan im;          // base 0
  uint64_t arena_bytes;
  uint64_t fit;          // fixed form: image k fits the arena iff k < fit (resend::fit_count)
  const uint32_t *conn;
  const tcpck_snd_state *snd;
  uint8_t *keep_out;     // d_keep, may be NULL
  uint8_t *keep;         // the scratch's keep bytes
  uint32_t *totals;      // the scratch's block totals
  uint32_t n_conns;
};

// Image k of the queue: whether its bytes may be touched at all, and where they are.
template <bool FIXED>
__device__ __forceinline__ bool image_at(const MarkArgs &a, uint32_t k, uint64_t &off) {
  off = a.im.start<FIXED>(k);  // (fixed form: used only when k < fit: no overflow then)
  if constexpr (FIXED) {
    return k < a.fit;
  } else {
    const uint32_t ln = a.im.length<FIXED>(k);
    return !((off | ln) & 1u) && ln >= resend::kMinImage && off <= a.arena_bytes && ln <= a.arena_bytes - off;
  }
}

template <int MODE, int RULE, bool FIXED>
__global__ void __launch_bounds__(compact::kBlock) resend_mark_kernel(MarkArgs a) {
  __shared__ uint32_t wave_total[compact::kWaves];
  const uint32_t first = compact::first_image();
  uint32_t n = 0;
#pragma unroll
  for (uint32_t i = 0; i < kChunks; ++i) {
    const uint32_t k = first + 64u * i;
    bool keep = false;
    if (k < a.im.count) {
      uint64_t off;
      const bool fits = image_at<FIXED>(a, k, off);
      const uint32_t c = a.conn ? a.conn[k] : 0u;
      if (fits && c < a.n_conns) {  // (TCPCK_CONN_NONE is >= every n_conns: the dead weak_ptr)
        const u32x4 st = *reinterpret_cast<const u32x4 *>(a.snd + c);  // snd_una, rcv_nxt, flags, reserved
        if (!(st.z & TCPCK_SND_CLOSED)) {
          uint16_t *w = reinterpret_cast<uint16_t *>(a.im.arena + off);  // even offsets: u16-aligned
          const uint32_t seq =
              __builtin_bswap32(w[resend::kWordSeq] | static_cast<uint32_t>(w[resend::kWordSeq + 1]) << 16);
          const uint32_t edge = ((w[resend::kWordFlags] >> 8) & resend::kSynFin) ? 1u : 0u;
          if constexpr (RULE == TCPCK_RESEND_REF) {
            keep = st.x < seq + edge;  // plain unsigned compare, u32 wrap of seq + 1, as the reference
          } else {
            const uint32_t n_seq = __builtin_bswap16(w[resend::kWordTcpLength]) + edge;
            keep = n_seq > 0 && static_cast<int32_t>(seq + n_seq - st.x) > 0;
          }
          if (keep) {
            const uint16_t o0 = w[resend::kWordAck], o1 = w[resend::kWordAck + 1], cs = w[resend::kWordChecksum];
            const uint32_t net = __builtin_bswap32(st.y);  // htonl(rcv_nxt) stored raw
            const uint16_t n0 = static_cast<uint16_t>(net), n1 = static_cast<uint16_t>(net >> 16);
            w[resend::kWordAck] = n0;
            w[resend::kWordAck + 1] = n1;
            w[resend::kWordChecksum] = dev::update_ack<MODE>(cs, o0, o1, n0, n1);
          }
        }
      }
      a.keep[k] = keep;
      if (a.keep_out) a.keep_out[k] = keep;
    }
    n += __popcll(__ballot(keep));
  }
  compact::store_block_total(wave_total, n, a.totals);
}

struct EmitArgs {
  ImageSpan im;             // arena unused, base 0
  const uint8_t *keep;
  const uint32_t *block_offsets;
  const uint32_t *conn;
  uint64_t *out_offsets;
  uint32_t *out_lengths, *out_conn, *src;
  uint64_t out_cap;
};

__global__ void __launch_bounds__(compact::kBlock) resend_emit_kernel(EmitArgs a) {
  __shared__ uint32_t wave_total[compact::kWaves];
  const uint32_t first = compact::first_image();
  bool keep[kChunks];
  uint64_t ballot[kChunks];
  uint32_t n = 0;
#pragma unroll
  for (uint32_t i = 0; i < kChunks; ++i) {
    const uint32_t k = first + 64u * i;
    keep[i] = k < a.im.count && a.keep[k] != 0;
    ballot[i] = __ballot(keep[i]);
    n += __popcll(ballot[i]);
  }
  uint32_t at = a.block_offsets[blockIdx.x] + compact::waves_before(wave_total, n);  // kept before this block, this wave
#pragma unroll
  for (uint32_t i = 0; i < kChunks; ++i) {
    const uint32_t k = first + 64u * i;
    const uint32_t j = at + compact::lanes_below(ballot[i]);
    at += __popcll(ballot[i]);
    if (!keep[i] || j >= a.out_cap) continue;
    if (a.out_offsets) a.out_offsets[j] = a.im.start(k);
    if (a.out_lengths) a.out_lengths[j] = a.im.length(k);
    if (a.out_conn) a.out_conn[j] = a.conn ? a.conn[k] : 0u;
    if (a.src) a.src[j] = k;
  }
}

template <int MODE, int RULE>
void launch_mark(const MarkArgs &a, uint32_t blocks, hipStream_t stream) {
  if (!a.im.is_fixed()) {
    hipLaunchKernelGGL((resend_mark_kernel<MODE, RULE, false>), dim3(blocks), dim3(compact::kBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((resend_mark_kernel<MODE, RULE, true>), dim3(blocks), dim3(compact::kBlock), 0, stream, a);
  }
}

}  // namespace

// The three launches; arguments valid, device selected, 0 < count <= 2^31.
static hipError_t launch_resend(int mode, int rule, MarkArgs m, EmitArgs e, uint64_t *d_count, hipStream_t stream) {
  // one launch covers every queue the entry point accepts: 2^31 images are 2^21
  // blocks, and every image and survivor index fits in a u32
  const uint32_t blocks = static_cast<uint32_t>(reply::blocks_for(m.im.count));
  if (mode == TCPCK_MODE_REF) {
    rule == TCPCK_RESEND_REF ? launch_mark<kRef, TCPCK_RESEND_REF>(m, blocks, stream)
                             : launch_mark<kRef, TCPCK_RESEND_SERIAL>(m, blocks, stream);
  } else {
    rule == TCPCK_RESEND_REF ? launch_mark<kRfc1071, TCPCK_RESEND_REF>(m, blocks, stream)
                             : launch_mark<kRfc1071, TCPCK_RESEND_SERIAL>(m, blocks, stream);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  err = compact::launch_scan_totals(m.totals, blocks, d_count, stream);
  if (err != hipSuccess) return err;
  if (!e.out_offsets && !e.out_lengths && !e.out_conn && !e.src) return hipSuccess;  // no list asked for
  hipLaunchKernelGGL(resend_emit_kernel, dim3(blocks), dim3(compact::kBlock), 0, stream, e);
  return hipGetLastError();
}

}  // namespace tcpck

using tcpck::api::DeviceGuard;
using tcpck::api::hip_status;

extern "C" int tcpck_resend_scratch_bytes(uint64_t count, size_t *bytes) {
  if (!bytes || count > tcpck::resend::kMaxCount) return TCPCK_EINVAL;
  *bytes = tcpck::resend::scratch_bytes(count);
  return TCPCK_OK;
}

extern "C" int tcpck_batch_resend(tcpck_ctx *ctx, int mode, int rule, void *d_arena, uint64_t arena_bytes,
                                  uint64_t stride, uint32_t len, const uint64_t *d_offsets, const uint32_t *d_lengths,
                                  const uint32_t *d_conn, const tcpck_snd_state *d_snd, uint32_t n_conns, uint64_t count,
                                  uint8_t *d_keep, uint64_t *d_out_offsets, uint32_t *d_out_lengths,
                                  uint32_t *d_out_conn, uint32_t *d_src, uint64_t out_cap, uint64_t *d_count,
                                  void *d_scratch, tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  const int rc = tcpck::resend::check(mode, rule, d_arena, stride, len, d_offsets, d_lengths, d_conn, d_snd, n_conns,
                                      count, d_out_offsets, d_out_lengths, d_out_conn, d_src, d_count);
  if (rc != TCPCK_OK) return rc;
  if (count > 0 && !d_scratch) return TCPCK_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_scratch) & 15) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (count == 0) return d_count ? hip_status(hipMemsetAsync(d_count, 0, sizeof(uint64_t), s)) : TCPCK_OK;
  uint8_t *scratch = static_cast<uint8_t *>(d_scratch);
  uint32_t *totals = reinterpret_cast<uint32_t *>(scratch);
  uint8_t *keep = scratch + tcpck::resend::totals_bytes(count);
  tcpck::MarkArgs m{};
  m.im = {static_cast<uint8_t *>(d_arena), d_offsets, d_lengths, stride, 0, count, len};
  m.arena_bytes = arena_bytes;
  m.fit = d_offsets ? 0 : tcpck::resend::fit_count(arena_bytes, stride, len);
  m.conn = d_conn;
  m.snd = d_snd;
  m.keep_out = d_keep;
  m.keep = keep;
  m.totals = totals;
  m.n_conns = n_conns;
  tcpck::EmitArgs e{};
  e.im = m.im;
  e.keep = keep;
  e.block_offsets = totals;
  e.conn = d_conn;
  e.out_offsets = d_out_offsets;
  e.out_lengths = d_out_lengths;
  e.out_conn = d_out_conn;
  e.src = d_src;
  e.out_cap = out_cap;
  return hip_status(tcpck::launch_resend(mode, rule, m, e, d_count, s));
}
