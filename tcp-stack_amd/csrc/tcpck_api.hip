// tcpck_api.hip -- the C-ABI of libtcpck.so (declared in include/tcpck.h).
//
// Replaces, for batches, the reference's per-packet checksum
// (filixi/TCP-stack include/tcp-header.h:252-263) at its call sites
// src/socket-manager.cc:9-10, include/socket-manager.h:259-260 (send: insert)
// and include/socket-manager.h:182 (receive: verify).  See include/tcpck.h.
//
// Ownership and threading: callers own every buffer; the hot
// batch calls allocate nothing and only enqueue work on the caller's stream;
// the current HIP device of the calling thread is saved and restored around
// every call (no hidden global device state).
//
// Here: the context, the single-image host calls, the thin wrappers of the
// batch calls and the calls that launch one kernel themselves.  The batch
// router is tcpck_router.hip, the host-memory (end-to-end) batches are
// tcpck_host_batch.hip.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "tcpck.h"
#include "tcpck_tuning.h"
#include "tcpck_internal.h"
#include "tcpck_api_internal.h"

using tcpck::api::DeviceGuard;
using tcpck::api::Hooks;
using tcpck::api::hip_status;

namespace tcpck {
namespace api {

int hip_status(hipError_t e) { return e == hipSuccess ? TCPCK_OK : TCPCK_EHIP - static_cast<int>(e); }

DeviceGuard::DeviceGuard(int device) {
  // A stale error left in the thread's last-error slot by an earlier failed
  // HIP call -- the caller's, or e.g. tcpck_device_supported(-1) -- would be
  // read back by the launchers' hipGetLastError() as this call's launch
  // status (found by tests/cpp/abi_host_test.cc): clear it first.
  (void)hipGetLastError();
  if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
  if (prev_ != device) ok_ = hipSetDevice(device);
}

DeviceGuard::~DeviceGuard() {
  if (prev_ >= 0) (void)hipSetDevice(prev_);
}

}  // namespace api
}  // namespace tcpck

namespace {

// ---- host single-image path (product code, not the oracle) ---------------
// The exact sum of the image's LE u16 words is tcpck::host::word_sum
// (tcpck_host.cc: AVX2 where the CPU has it, else SWAR); REF needs it mod
// 2^16, RFC 1071 mod 0xFFFF with zero-ness.
uint16_t finish_host(uint64_t total, int mode) {
  if (mode == TCPCK_MODE_REF) return static_cast<uint16_t>(~total);  // tcp-header.h:262
  while (total >> 16) total = (total & 0xFFFF) + (total >> 16);
  return static_cast<uint16_t>(~total);
}

// Everything the context owns on the device: the router's scratch slots and
// pipe stream, the probe library's side state, the host batches' staging.
void free_device_state(tcpck_ctx *ctx) {
  for (auto &slot : ctx->scratch) {
    if (slot.ev) {
      (void)hipEventSynchronize(slot.ev);
      (void)hipEventDestroy(slot.ev);
    }
    if (slot.buf) (void)hipFree(slot.buf);
  }
  if (ctx->pipe) {
    (void)hipStreamSynchronize(ctx->pipe);
    (void)hipStreamDestroy(ctx->pipe);
  }
  for (auto &ev : ctx->pipe_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->probe_side) (void)hipFree(ctx->probe_side);
  if (ctx->side) {
    (void)hipEventDestroy(ctx->fork);
    (void)hipEventDestroy(ctx->join);
    (void)hipStreamDestroy(ctx->side);
  }
  for (int i = 0; i < 2; ++i) {
    if (ctx->stage[i]) (void)hipFree(ctx->stage[i]);
    if (ctx->stage_out[i]) (void)hipFree(ctx->stage_out[i]);
    if (ctx->stage_off[i]) (void)hipFree(ctx->stage_off[i]);
    if (ctx->stage_len[i]) (void)hipFree(ctx->stage_len[i]);
    if (ctx->s[i]) (void)hipStreamDestroy(ctx->s[i]);
  }
}

}  // namespace

extern "C" {

int tcpck_abi_version(void) { return TCPCK_ABI_VERSION; }

const char *tcpck_strerror(int status) {
  if (status == TCPCK_OK) return "ok";
  if (status == TCPCK_EINVAL) return "invalid argument (odd length/offset, null pointer, overflow)";
  if (status == TCPCK_ENOMEM) return "out of memory";
  if (status == TCPCK_ENODEV) return "no such HIP device";
  if (status <= TCPCK_EHIP) return hipGetErrorString(static_cast<hipError_t>(TCPCK_EHIP - status));
  return "unknown status";
}

int tcpck_device_supported(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    (void)hipGetLastError();  // no stale error for the caller's next HIP call
    return 0;
  }
  return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int tcpck_ctx_create(int device, tcpck_ctx **out) {
  if (!out) return TCPCK_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    (void)hipGetLastError();
    return TCPCK_ENODEV;
  }
  if (!tcpck_device_supported(device)) return TCPCK_ENODEV;  // gfx950 code object only
  auto *ctx = new (std::nothrow) tcpck_ctx;
  if (!ctx) return TCPCK_ENOMEM;
  ctx->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    ctx->num_cus = prop.multiProcessorCount;
  // (the results scratch of out-less FILLs is allocated on first use: take_scratch, tcpck_router.hip)
  *out = ctx;
  return TCPCK_OK;
}

int tcpck_ctx_destroy(tcpck_ctx *ctx) {
  if (!ctx) return TCPCK_EINVAL;
  {
    DeviceGuard g(ctx->device);
    free_device_state(ctx);
  }
  delete ctx;
  return TCPCK_OK;
}

int tcpck_ctx_device(const tcpck_ctx *ctx) { return ctx ? ctx->device : TCPCK_EINVAL; }

int tcpck_ctx_set_chunk_bytes(tcpck_ctx *ctx, uint64_t bytes) {
  if (!ctx || bytes < 4096) return TCPCK_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->chunk_bytes = bytes;
  return TCPCK_OK;
}

// ---- single image, host ----------------------------------------------------
int tcpck_checksum16(const void *image, size_t len, int mode, uint16_t *out) {
  if ((!image && len) || !out || (len & 1) ||
      (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071))
    return TCPCK_EINVAL;
  *out = finish_host(tcpck::host::word_sum(static_cast<const uint8_t *>(image), len), mode);
  return TCPCK_OK;
}

int tcpck_fill16(void *image, size_t len, int mode, uint16_t *out) {
  // validate everything before the image is touched: a rejected call leaves bytes 28-29 as they were
  if (!image || len < 30 || (len & 1) || (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071))
    return TCPCK_EINVAL;
  auto *b = static_cast<uint8_t *>(image);
  b[28] = 0;  // socket-manager.cc:9
  b[29] = 0;
  uint16_t c;
  int rc = tcpck_checksum16(image, len, mode, &c);  // socket-manager.cc:10
  if (rc) return rc;
  std::memcpy(b + 28, &c, 2);
  if (out) *out = c;
  return TCPCK_OK;
}

uint16_t tcpck_update16(uint16_t checksum, uint16_t old_word, uint16_t new_word, int mode) {
  if (mode == TCPCK_MODE_REF) {
    // stored C = ~S (mod 2^16)  =>  C' = ~(S - old + new)
    const uint16_t s = static_cast<uint16_t>(~checksum);
    return static_cast<uint16_t>(~static_cast<uint16_t>(s - old_word + new_word));
  }
  // RFC 1624 eqn. 3: C' = ~(~C + ~m + m') in one's complement arithmetic.
  uint32_t s = static_cast<uint16_t>(~checksum) + static_cast<uint32_t>(static_cast<uint16_t>(~old_word)) +
               new_word;
  s = (s & 0xFFFF) + (s >> 16);
  s = (s & 0xFFFF) + (s >> 16);
  if (s == 0) s = 0xFFFF;  // a real (non-all-zero) image never folds to +0
  return static_cast<uint16_t>(~s);
}

// ---- batched, device-resident -------------------------------------------------
int tcpck_batch_fixed(tcpck_ctx *ctx, int op, int mode, void *d_arena, uint64_t stride,
                      uint32_t len, uint64_t count, void *d_out, tcpck_stream stream) {
  return tcpck::api::batch_fixed_ex(ctx, op, mode, d_arena, stride, len, count, d_out, TCPCK_KERNEL_AUTO, 0,
                                    static_cast<hipStream_t>(stream), Hooks{});
}

int tcpck_batch_var(tcpck_ctx *ctx, int op, int mode, void *d_arena, const uint64_t *d_offsets,
                    const uint32_t *d_lengths, uint64_t count, void *d_out,
                    const tcpck_layout *layout, tcpck_stream stream) {
  return tcpck::api::batch_var_ex(ctx, op, mode, d_arena, d_offsets, d_lengths, count, d_out, layout,
                                  TCPCK_KERNEL_AUTO, 0, static_cast<hipStream_t>(stream), Hooks{});
}

// (tcpck_batch_fixed_ex / tcpck_batch_var_ex / tcpck_batch_receive_ex, the
// tuning entry points: tcpck_ex.hip, and tcpck_ex_probe.hip in the probe library;
// tcpck_host_batch_*: tcpck_host_batch.hip)

// ---- batched retransmit: ACK rewrite + incremental update ----------------------
int tcpck_batch_set_ack(tcpck_ctx *ctx, int mode, void *d_arena, const uint64_t *d_offsets, uint64_t stride,
                        uint64_t count, const uint32_t *d_acks, uint32_t ack, uint16_t *d_out,
                        tcpck_stream stream) {
  if (!ctx || (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || (reinterpret_cast<uintptr_t>(d_arena) & 1)) return TCPCK_EINVAL;
  if (!d_offsets && !tcpck::api::valid_fixed_slots(stride, 30, count)) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::AckArgs a{};
  a.im = {static_cast<uint8_t *>(d_arena), d_offsets, nullptr, stride, 0, count, 0};
  a.acks = d_acks;
  a.ack = ack;
  a.out = d_out;
  return hip_status(tcpck::launch_set_ack(mode, a, static_cast<uint32_t>(ctx->num_cus),
                                          static_cast<hipStream_t>(stream)));
}

// ---- receive batch: verdicts + host-order headers ------------------------------------
int tcpck_batch_receive(tcpck_ctx *ctx, int mode, void *d_arena, uint64_t stride, uint32_t len,
                        const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, uint8_t *d_ok,
                        void *d_hdr, const tcpck_layout *layout, tcpck_stream stream) {
  return tcpck::api::batch_receive_ex(ctx, mode, d_arena, stride, len, d_offsets, d_lengths, count, d_ok, d_hdr,
                                      layout, TCPCK_KERNEL_AUTO, 0, static_cast<hipStream_t>(stream), Hooks{});
}

// ---- header byte order: TcpHeaderN2H / TcpHeaderH2N in place -----------------------
int tcpck_batch_header_swap(tcpck_ctx *ctx, void *d_arena, const uint64_t *d_offsets, uint64_t stride,
                            uint64_t count, tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || (reinterpret_cast<uintptr_t>(d_arena) & 1)) return TCPCK_EINVAL;
  if (count > (UINT64_MAX >> 4)) return TCPCK_EINVAL;
  if (!d_offsets && !tcpck::api::valid_fixed_slots(stride, TCPCK_HEADER_BYTES, count)) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::HeaderArgs a{};
  a.im = {static_cast<uint8_t *>(d_arena), d_offsets, nullptr, stride, 0, count, 0};
  return hip_status(tcpck::launch_header_swap(a, static_cast<uint32_t>(ctx->num_cus),
                                              static_cast<hipStream_t>(stream)));
}

// ---- batched segmentation: send stream -> checksummed images --------------------
int tcpck_batch_segment(tcpck_ctx *ctx, int mode, const void *d_payload, uint64_t payload_bytes, uint32_t seg,
                        const void *hdr, uint32_t seq0, void *d_images, uint64_t stride, uint16_t *d_out,
                        tcpck_stream stream) {
  return tcpck_batch_segment_ex(ctx, mode, d_payload, payload_bytes, seg, hdr, seq0, d_images, stride, d_out, 0,
                                stream);
}

int tcpck_batch_segment_ex(tcpck_ctx *ctx, int mode, const void *d_payload, uint64_t payload_bytes, uint32_t seg,
                           const void *hdr, uint32_t seq0, void *d_images, uint64_t stride, uint16_t *d_out,
                           int param, tcpck_stream stream) {
  if (!ctx || (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071)) return TCPCK_EINVAL;
  if (payload_bytes == 0) return TCPCK_OK;
  if (!d_payload || !d_images || !hdr || (payload_bytes & 1)) return TCPCK_EINVAL;
  if (seg < 4 || seg > 65532 || (seg & 3) || (stride & 15) || stride < 32ull + seg || stride > (1u << 24))
    return TCPCK_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d_payload) & 3) || (reinterpret_cast<uintptr_t>(d_images) & 15))
    return TCPCK_EINVAL;
  const uint64_t n = (payload_bytes + seg - 1) / seg;
  if (n > UINT64_MAX / stride) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::SegmentArgs a{};
  a.payload = static_cast<const uint8_t *>(d_payload);
  a.images = static_cast<uint8_t *>(d_images);
  a.payload_bytes = payload_bytes;
  a.count = n;
  a.out = d_out;
  a.seg = seg;
  a.stride = static_cast<uint32_t>(stride);
  std::memcpy(a.hdr, hdr, 32);
  a.seq0 = seq0;
  return hip_status(tcpck::launch_segment(mode, param & 0xFF, a, static_cast<uint32_t>(param >> 16) & 0xFFFFu,
                                          static_cast<uint32_t>(ctx->num_cus), static_cast<hipStream_t>(stream)));
}

// ---- memory helpers -----------------------------------------------------------
int tcpck_host_alloc(size_t bytes, void **out) {
  if (!out) return TCPCK_EINVAL;
  *out = nullptr;
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? TCPCK_OK : TCPCK_ENOMEM;
}

int tcpck_host_free(void *p) { return hip_status(hipHostFree(p)); }

int tcpck_device_alloc(tcpck_ctx *ctx, size_t bytes, void **out) {
  if (!ctx || !out) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  *out = nullptr;
  return hipMalloc(out, bytes) == hipSuccess ? TCPCK_OK : TCPCK_ENOMEM;
}

int tcpck_device_free(tcpck_ctx *ctx, void *p) {
  if (!ctx) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  return hip_status(hipFree(p));
}

int tcpck_memcpy_h2d(tcpck_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  return hip_status(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
}

int tcpck_memcpy_d2h(tcpck_ctx *ctx, void *dst, const void *src, size_t bytes) {
  if (!ctx) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  return hip_status(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
}

int tcpck_stream_sync(tcpck_ctx *ctx, tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  return hip_status(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
}

}  // extern "C"

