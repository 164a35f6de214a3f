// tcpck_demux.hip -- the receive demultiplexer's device side: the connection
// table's image (allocation at create, upload at commit) and the batched lookup
// tcpck_batch_demux (include/tcpck.h).
//
// Reference (filixi/TCP-stack), per packet:
//   SocketManager::ReceivePacket            include/socket-manager.h:181-208
//     host_port = DestinationPort(), peer_ip = SourceAddress(), peer_port =
//     SourcePort(); Syn() && !Ack(): FindInternal(host_port, 0, 0), the
//     listener; else FindInternal of the full key (:187-196, :235-245) -- an
//     unordered_map find under the manager's mutex.  The destination address
//     is not part of the key.
// The host mirror and the image's layout are tcpck_conn_table.cc / .h.
//
// The kernel: one image per lane.  Lane k reads header k of the dense 32-B
// host-order array -- dword 0 (source address), dword 3 (source | destination
// port << 16) and dword 6 (flags in bits 8-15), three loads over the same 2 KiB
// of consecutive lines per wave; the key is hashed as the host does and the lane
// walks its probe run, one 16-B slot load per step, until the key or an empty
// slot.  The table (16 B x slots, 2 MiB at 64K connections) stays in L2; the
// run is a chain of dependent loads that occupancy hides, so the kernel keeps
// its registers low and holds nothing across the loop but the key.  The ids
// leave as one coalesced dword store per lane.  The loop is bounded by the
// slot count whatever the image holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "tcpck_api_internal.h"
#include "tcpck_conn_table.h"

namespace tcpck {

namespace {

using conn::Slot;

constexpr uint32_t kDemuxBlock = 256;
// images per launch: the grid stays below 2^23 blocks and every index in u32
constexpr uint64_t kDemuxLaunch = 1ull << 30;

constexpr uint32_t kAck = 0x08, kSyn = 0x40;  // header byte 25 (tcp-header.h:122-162)

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kDemuxBlock) demux_kernel(const uint8_t *__restrict__ hdr,
                                                            const Slot *__restrict__ table, uint32_t mask,
                                                            uint32_t *__restrict__ conn_out, uint32_t count) {
  const uint32_t k = blockIdx.x * kDemuxBlock + threadIdx.x;
  if (k >= count) return;
  const uint32_t *h = reinterpret_cast<const uint32_t *>(hdr + 32ull * k);  // (4-B aligned)
  const uint32_t flags = (h[6] >> 8) & 0xFFu;
  uint32_t peer_ip = h[0], ports = h[3];
  if ((flags & (kSyn | kAck)) == kSyn) {  // Syn() && !Ack(): the listener (host_port, 0, 0)
    peer_ip = 0;
    ports &= 0xFFFF0000u;
  }
  uint32_t i = conn::hash(peer_ip, ports) & mask;
  uint32_t id = TCPCK_CONN_NONE;
  for (uint32_t n = 0; n <= mask; ++n) {  // at most every slot once
    const u32x4v s = *reinterpret_cast<const u32x4v *>(table + i);  // {peer_ip, ports, id, used}
    if (!s.w) break;
    if (s.x == peer_ip && s.y == ports) {
      id = s.z;
      break;
    }
    i = (i + 1) & mask;
  }
  conn_out[k] = id;
}

}  // namespace

hipError_t launch_demux(const tcpck_conn_table *t, const uint8_t *d_hdr, uint64_t count, uint32_t *d_conn,
                        hipStream_t stream) {
  for (uint64_t at = 0; at < count; at += kDemuxLaunch) {
    const uint32_t n = static_cast<uint32_t>(std::min(kDemuxLaunch, count - at));
    const uint32_t blocks = (n + kDemuxBlock - 1) / kDemuxBlock;
    hipLaunchKernelGGL(demux_kernel, dim3(blocks), dim3(kDemuxBlock), 0, stream, d_hdr + 32 * at, t->d_image,
                       t->slots - 1, d_conn + at, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace tcpck

using tcpck::api::DeviceGuard;
using tcpck::api::hip_status;

extern "C" int tcpck_conn_table_create(tcpck_ctx *ctx, uint32_t max_conns, tcpck_conn_table **out) {
  if (!out || max_conns == 0 || max_conns > tcpck::conn::kMaxConns) return TCPCK_EINVAL;
  tcpck_conn_table *t = new (std::nothrow) tcpck_conn_table;
  if (!t) return TCPCK_ENOMEM;
  t->max_conns = max_conns;
  t->slots = tcpck::conn::kMinSlots;
  while (t->slots < 2 * max_conns) t->slots *= 2;
  try {
    t->mirror.assign(t->slots, tcpck::conn::Slot{0, 0, 0, 0});
    t->image.reserve(t->slots);
  } catch (const std::bad_alloc &) {
    delete t;
    return TCPCK_ENOMEM;
  }
  if (ctx) {
    DeviceGuard g(ctx->device);
    hipError_t e = g.status();
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&t->d_image), sizeof(tcpck::conn::Slot) * t->slots);
    if (e != hipSuccess) {
      delete t;
      return e == hipErrorOutOfMemory ? TCPCK_ENOMEM : hip_status(e);
    }
    t->device = ctx->device;
  }
  *out = t;
  return TCPCK_OK;
}

extern "C" int tcpck_conn_table_destroy(tcpck_conn_table *t) {
  if (!t) return TCPCK_EINVAL;
  hipError_t e = hipSuccess;
  if (t->d_image) {
    DeviceGuard g(t->device);
    e = g.status();
    if (e == hipSuccess) e = hipFree(t->d_image);  // (waits for the launches that read it)
  }
  delete t;
  return hip_status(e);
}

extern "C" int tcpck_conn_table_commit(tcpck_conn_table *t, tcpck_stream stream) {
  if (!t) return TCPCK_EINVAL;
  uint32_t longest = 0;
  uint64_t wrapped = 0;
  tcpck::conn::rebuild(t->mirror, t->image, longest, wrapped);  // (capacity reserved at create)
  if (t->d_image) {
    DeviceGuard g(t->device);
    if (g.status() != hipSuccess) return hip_status(g.status());
    hipStream_t s = static_cast<hipStream_t>(stream);
    // in stream order after the launches already enqueued there; the host
    // copy is reused by the next commit, so wait for the upload
    hipError_t e = hipMemcpyAsync(t->d_image, t->image.data(), sizeof(tcpck::conn::Slot) * t->slots,
                                  hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e);
  }
  t->committed = true;
  t->image_entries = t->entries;
  t->image_longest = longest;
  t->image_wrapped = wrapped;
  return TCPCK_OK;
}

extern "C" int tcpck_batch_demux(tcpck_ctx *ctx, const tcpck_conn_table *t, const void *d_hdr, uint64_t count,
                                 uint32_t *d_conn, tcpck_stream stream) {
  if (!ctx || !t) return TCPCK_EINVAL;
  if (!t->d_image || t->device != ctx->device || !t->committed) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_hdr || !d_conn) return TCPCK_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d_hdr) & 3) || (reinterpret_cast<uintptr_t>(d_conn) & 3)) return TCPCK_EINVAL;
  if (count > UINT64_MAX / 32) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  return hip_status(tcpck::launch_demux(t, static_cast<const uint8_t *>(d_hdr), count, d_conn,
                                        static_cast<hipStream_t>(stream)));
}
