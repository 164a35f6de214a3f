// tcpck_reply.hip -- the batched reply builder's device side: tcpck_batch_reply
// (include/tcpck.h) turns the receive planners' verdicts into a dense ring of
// 32-byte, checksummed, network-order ACK / RST datagrams.
//
// Reference (filixi/TCP-stack), per datagram:
//   ACK  SocketInternal::SendAck            include/socket-internal.h:293-299
//          MakeTcpPacket(0), AckHeader(seq, ack, wnd) (:24-30)
//        SocketInternal::SendPacket         src/socket-internal.cc:35-42
//          SetSource / SetDestination (:52-60), TcpHeaderH2N
//        SocketManager::SendPacket          src/socket-manager.cc:6-12
//          Checksum() = 0; Checksum() = CalculateChecksum(*p)
//   RST  SocketManager::ReceivePacket       include/socket-manager.h:201-207
//          MakeTcpPacket(0), RstHeader(packet header, ...) (:43-50),
//          TcpHeaderH2N, the checksum; no SetSource / SetDestination.
// The host twin is tcpck_reply_host.cc; both follow the rule stated at
// tcpck_batch_reply in include/tcpck.h.
//
// The shape is a stable stream compaction with a fixed 32-B payload per
// survivor, in three launches on the caller's stream; no block waits for
// another block and no atomic orders anything:
//   count  one block per kImagesPerBlock images, one image per lane and
//          kReplyChunks chunks of 64 per wave: the reply predicate (verdict
//          byte, and for an ACK the connection id against n_conns), a wave
//          ballot per chunk, the block's total into d_scratch[block];
//   scan   (tcpck_compact.h, shared with tcpck_resend_queue.hip) ONE block of
//          kScanBlock threads turns the block totals into exclusive offsets in place, kScanBlock totals per step with a
//          running carry (the loop is bounded by the block count, a launch
//          argument), and stores the grand total to *d_count;
//   emit   the count pass's predicate again; a replying lane's index is
//          d_scratch[block] + the waves before it in the block (LDS) + the
//          chunks before it in the wave + mbcnt of the chunk's ballot.  The
//          lane builds its eight dwords in registers -- the template of its
//          connection as two 16-B loads (templates stay in L2), the ACK
//          number byte-reversed by one v_perm, the ACK bit; or, for an RST,
//          zeros, the sequence number and the RST bit -- sums the sixteen
//          words as the other kernels do (tcpck_device.h accumulate / finish)
//          and stores the record as two 16-B stores at 32 j, j < reply_cap.
//          Consecutive replying lanes write consecutive records.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tcpck_api_internal.h"
#include "tcpck_compact.h"
#include "tcpck_device.h"
#include "tcpck_reply.h"

namespace tcpck {

namespace {

using dev::u32x4;

// the compaction's geometry, scan and index arithmetic: tcpck_compact.h
constexpr uint32_t kReplyBlock = compact::kBlock;
constexpr uint32_t kReplyWaves = compact::kWaves;
constexpr uint32_t kReplyChunks = compact::kChunks;  // chunks of 64 images per wave
using compact::lanes_below;

constexpr uint32_t kNone = 0, kAck = 1, kRst = 2;

// What image k is answered with, and (for an ACK) its connection in `c`.
__device__ __forceinline__ uint32_t reply_kind(const uint8_t *__restrict__ verdict, const uint32_t *__restrict__ conn,
                                               uint32_t n_conns, uint32_t k, uint32_t count, uint32_t &c) {
  c = 0;
  if (k >= count) return kNone;
  const uint32_t v = verdict[k];
  if (v & TCPCK_RCV_RST) return kRst;
  if (!(v & TCPCK_RCV_SEND_ACK)) return kNone;
  if (conn) c = conn[k];
  return c < n_conns ? kAck : kNone;  // (TCPCK_CONN_NONE is >= every n_conns)
}

__global__ void __launch_bounds__(kReplyBlock) reply_count_kernel(const uint8_t *__restrict__ verdict,
                                                                  const uint32_t *__restrict__ conn, uint32_t n_conns,
                                                                  uint32_t count, uint32_t *__restrict__ totals) {
  __shared__ uint32_t wave_total[kReplyWaves];
  const uint32_t first = compact::first_image();
  uint32_t n = 0;
#pragma unroll
  for (uint32_t i = 0; i < kReplyChunks; ++i) {
    uint32_t c;
    n += __popcll(__ballot(reply_kind(verdict, conn, n_conns, first + 64u * i, count, c) != kNone));
  }
  compact::store_block_total(wave_total, n, totals);
}

template <int MODE>
__device__ __forceinline__ void store_reply(uint8_t *__restrict__ replies, uint32_t j, u32x4 lo, u32x4 hi) {
  hi.w &= 0xFFFF0000u;  // Checksum() = 0 (bytes 28-29), then the sum of the sixteen words
  uint32_t acc = 0;
  acc = dev::accumulate<MODE>(acc, lo.x);
  acc = dev::accumulate<MODE>(acc, lo.y);
  acc = dev::accumulate<MODE>(acc, lo.z);
  acc = dev::accumulate<MODE>(acc, lo.w);
  acc = dev::accumulate<MODE>(acc, hi.x);
  acc = dev::accumulate<MODE>(acc, hi.y);
  acc = dev::accumulate<MODE>(acc, hi.z);
  acc = dev::accumulate<MODE>(acc, hi.w);
  hi.w |= dev::finish<MODE>(acc);  // stored raw, as the reference
  u32x4 *out = reinterpret_cast<u32x4 *>(replies + 32ull * j);
  out[0] = lo;
  out[1] = hi;
}

template <int MODE>
__global__ void __launch_bounds__(kReplyBlock)
    reply_emit_kernel(const uint8_t *__restrict__ verdict, const uint32_t *__restrict__ ack,
                      const uint32_t *__restrict__ conn, const uint8_t *__restrict__ tmpl, uint32_t n_conns,
                      uint32_t count, const uint32_t *__restrict__ offsets, uint8_t *__restrict__ replies,
                      uint64_t reply_cap, uint32_t *__restrict__ src) {
  __shared__ uint32_t wave_total[kReplyWaves];
  const uint32_t first = compact::first_image();
  uint32_t kind[kReplyChunks], c[kReplyChunks];
  uint64_t ballot[kReplyChunks];
  uint32_t n = 0;
#pragma unroll
  for (uint32_t i = 0; i < kReplyChunks; ++i) {
    kind[i] = reply_kind(verdict, conn, n_conns, first + 64u * i, count, c[i]);
    ballot[i] = __ballot(kind[i] != kNone);
    n += __popcll(ballot[i]);
  }
  uint32_t at = offsets[blockIdx.x] + compact::waves_before(wave_total, n);  // replies before this block, this wave
#pragma unroll
  for (uint32_t i = 0; i < kReplyChunks; ++i) {
    const uint32_t k = first + 64u * i;
    const uint32_t j = at + lanes_below(ballot[i]);
    at += __popcll(ballot[i]);
    if (kind[i] == kNone || j >= reply_cap) continue;
    const uint32_t number = dev::n2h_dword(ack[k], 0x00010203u);  // htonl
    u32x4 lo{0, 0, 0, 0}, hi{0, 0, 0, 0};
    if (kind[i] == kAck) {  // (c[i] < n_conns: reply_kind)
      const u32x4 *t = reinterpret_cast<const u32x4 *>(tmpl + 32ull * c[i]);
      lo = t[0];
      hi = t[1];
      hi.y = number;     // bytes 20-23: AcknowledgementNumber
      hi.z |= 0x0800u;   // byte 25: ACK
    } else {
      hi.x = number;     // bytes 16-19: SequenceNumber = the image's acknowledgement number
      hi.z = 0x2000u;    // byte 25: RST
    }
    store_reply<MODE>(replies, j, lo, hi);
    if (src) src[j] = k;
  }
}

}  // namespace

// The three launches; arguments valid, device selected, 0 < count <= 2^31.
static hipError_t launch_reply(int mode, const uint8_t *d_verdict, const uint32_t *d_ack, const uint32_t *d_conn,
                               const uint8_t *d_tmpl, uint32_t n_conns, uint64_t count, uint8_t *d_replies,
                               uint64_t reply_cap, uint32_t *d_src, uint64_t *d_count, uint32_t *d_scratch,
                               hipStream_t stream) {
  // one launch covers every ring the entry point accepts: 2^31 images are 2^21
  // blocks, and every image and reply index fits in a u32
  const uint32_t n = static_cast<uint32_t>(count);
  const uint32_t blocks = static_cast<uint32_t>(reply::blocks_for(count));
  hipLaunchKernelGGL(reply_count_kernel, dim3(blocks), dim3(kReplyBlock), 0, stream, d_verdict, d_conn, n_conns, n,
                     d_scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = compact::launch_scan_totals(d_scratch, blocks, d_count, stream);
  if (e != hipSuccess) return e;
  if (mode == TCPCK_MODE_REF) {
    hipLaunchKernelGGL(reply_emit_kernel<kRef>, dim3(blocks), dim3(kReplyBlock), 0, stream, d_verdict, d_ack, d_conn,
                       d_tmpl, n_conns, n, d_scratch, d_replies, reply_cap, d_src);
  } else {
    hipLaunchKernelGGL(reply_emit_kernel<kRfc1071>, dim3(blocks), dim3(kReplyBlock), 0, stream, d_verdict, d_ack,
                       d_conn, d_tmpl, n_conns, n, d_scratch, d_replies, reply_cap, d_src);
  }
  return hipGetLastError();
}

}  // namespace tcpck

using tcpck::api::DeviceGuard;
using tcpck::api::hip_status;

extern "C" int tcpck_reply_scratch_bytes(uint64_t count, size_t *bytes) {
  if (!bytes || count > tcpck::reply::kMaxCount) return TCPCK_EINVAL;
  *bytes = tcpck::reply::scratch_bytes(count);
  return TCPCK_OK;
}

extern "C" int tcpck_batch_reply(tcpck_ctx *ctx, int mode, const uint8_t *d_verdict, const uint32_t *d_ack,
                                 const uint32_t *d_conn, const void *d_tmpl, uint32_t n_conns, uint64_t count,
                                 void *d_replies, uint64_t reply_cap, uint32_t *d_src, uint64_t *d_count,
                                 void *d_scratch, tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  const int rc = tcpck::reply::check(mode, d_verdict, d_ack, d_conn, d_tmpl, n_conns, count, d_replies, d_src, d_count);
  if (rc != TCPCK_OK) return rc;
  if (count > 0 && !d_scratch) return TCPCK_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_scratch) & 15) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (count == 0) return d_count ? hip_status(hipMemsetAsync(d_count, 0, sizeof(uint64_t), s)) : TCPCK_OK;
  return hip_status(tcpck::launch_reply(mode, d_verdict, d_ack, d_conn, static_cast<const uint8_t *>(d_tmpl), n_conns,
                                        count, static_cast<uint8_t *>(d_replies), reply_cap, d_src, d_count,
                                        static_cast<uint32_t *>(d_scratch), s));
}
