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
// every call (no hidden global device state).  The host-batch (end-to-end)
// calls use ctx-owned streams and staging and are serialised per ctx.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "tcpck.h"
#include "tcpck_tuning.h"
#include "tcpck_internal.h"
#include "tcpck_api_internal.h"

using tcpck::SegArgs;
using tcpck::api::DeviceGuard;
using tcpck::api::Fill;
using tcpck::api::Hdr;
using tcpck::api::Hooks;
using tcpck::api::Plan;
using tcpck::api::plan_fixed;
using tcpck::api::plan_var;
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

size_t out_elem(int op) { return op == TCPCK_OP_VERIFY ? 1 : 2; }

bool valid_op_mode(int op, int mode) {
  return (op == TCPCK_OP_CHECKSUM || op == TCPCK_OP_FILL || op == TCPCK_OP_VERIFY) &&
         (mode == TCPCK_MODE_REF || mode == TCPCK_MODE_RFC1071);
}
// device batches also take RECEIVE (VERIFY + TcpHeaderN2H)
bool valid_device_op_mode(int op, int mode) { return valid_op_mode(op == TCPCK_OP_RECEIVE ? TCPCK_OP_VERIFY : op, mode); }

// ---- host single-image path (product code, not the oracle) ---------------
// The exact sum of the image's LE u16 words is tcpck::host::word_sum
// (tcpck_host.cc: AVX2 where the CPU has it, else SWAR); REF needs it mod
// 2^16, RFC 1071 mod 0xFFFF with zero-ness.
uint16_t finish_host(uint64_t total, int mode) {
  if (mode == TCPCK_MODE_REF) return static_cast<uint16_t>(~total);  // tcp-header.h:262
  while (total >> 16) total = (total & 0xFFFF) + (total >> 16);
  return static_cast<uint16_t>(~total);
}

// Grows the host-batch staging buffers.  New buffers are allocated into
// temporaries and swapped in only when every allocation succeeded, so a failed
// (ENOMEM) request leaves the context's previous buffers and sizes intact and a
// later smaller request still runs on them.
int ensure_stage(tcpck_ctx *ctx, uint64_t bytes, uint64_t images) {
  if (!ctx->s[0]) {
    for (int i = 0; i < 2; ++i) {
      hipError_t e = hipStreamCreateWithFlags(&ctx->s[i], hipStreamNonBlocking);
      if (e != hipSuccess) return hip_status(e);
    }
  }
  if (bytes > ctx->stage_bytes) {
    if (bytes > UINT64_MAX - 16) return TCPCK_ENOMEM;
    uint8_t *fresh[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
      if (hipMalloc(&fresh[i], bytes + 16) != hipSuccess) {
        for (int j = 0; j < 2; ++j)
          if (fresh[j]) (void)hipFree(fresh[j]);
        (void)hipGetLastError();  // clear the allocation error so the caller's next launch check is clean
        return TCPCK_ENOMEM;
      }
    }
    for (int i = 0; i < 2; ++i) {
      if (ctx->stage[i]) (void)hipFree(ctx->stage[i]);
      ctx->stage[i] = fresh[i];
    }
    ctx->stage_bytes = bytes;
  }
  if (images > ctx->stage_images) {
    if (images > UINT64_MAX / 8) return TCPCK_ENOMEM;
    void *fresh[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    const uint64_t size[3] = {images * 2, images * 8, images * 4};
    for (int i = 0; i < 2; ++i) {
      for (int k = 0; k < 3; ++k) {
        if (hipMalloc(&fresh[i][k], size[k]) != hipSuccess) {
          for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 3; ++b)
              if (fresh[a][b]) (void)hipFree(fresh[a][b]);
          (void)hipGetLastError();
          return TCPCK_ENOMEM;
        }
      }
    }
    for (int i = 0; i < 2; ++i) {
      if (ctx->stage_out[i]) (void)hipFree(ctx->stage_out[i]);
      if (ctx->stage_off[i]) (void)hipFree(ctx->stage_off[i]);
      if (ctx->stage_len[i]) (void)hipFree(ctx->stage_len[i]);
      ctx->stage_out[i] = static_cast<uint8_t *>(fresh[i][0]);
      ctx->stage_off[i] = static_cast<uint64_t *>(fresh[i][1]);
      ctx->stage_len[i] = static_cast<uint32_t *>(fresh[i][2]);
    }
    ctx->stage_images = images;
  }
  return TCPCK_OK;
}

void free_stage(tcpck_ctx *ctx) {
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

// ---- the batch router: plan, then launch ---------------------------------
// tcpck_plan.h decides a batch once -- AUTO's kernel and param, FILL's and
// RECEIVE's form, whether the request is rejected (plan_fixed / plan_var; the
// policy and its measurements are in tcpck_plan.cc); the functions below
// launch a plan on the caller's buffers and decide nothing.

// FILL's field pass on `s`, or -- pipelined FILL (fill_pipelined) -- on `ps`
// after the event `pev` recorded on `s` behind the stream pass it reads.
hipError_t launch_patch_on(const tcpck::PatchArgs &pa, uint32_t num_cus, hipStream_t s, hipStream_t ps,
                           hipEvent_t pev) {
  if (ps) {
    hipError_t e = hipEventRecord(pev, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(ps, pev, 0);
    if (e != hipSuccess) return e;
    s = ps;
  }
  return tcpck::launch_patch_fields(pa, num_cus, s);
}

// The passes around a plan's stream kernel (launch_stream: that kernel on the
// batch), in the plan's order; `pa` and `h` are the batch's field pass and
// header pass.
template <typename LaunchStream>
hipError_t launch_plan(const Plan &p, tcpck::PatchArgs pa, const tcpck::HeaderArgs &h, uint32_t num_cus, hipStream_t s,
                       const Hooks &hk, hipStream_t ps, hipEvent_t pev, LaunchStream launch_stream) {
  hipError_t e = p.hdr == Hdr::kFirst ? tcpck::launch_header_swap(h, num_cus, s) : hipSuccess;
  if (e == hipSuccess) e = p.rejected ? hipErrorInvalidValue : launch_stream();
  if (e != hipSuccess) return e;
  if (p.field_pass()) {  // the fields the stream left: write-through 2-B stores (launch_patch_fields)
    pa.update = p.fill == Fill::kUpdate ? 1u : 0u;
    pa.reverse = hk.patch_reverse ? 1u : 0u;
    return launch_patch_on(pa, num_cus, s, ps, pev);
  }
  return p.hdr == Hdr::kAfter ? tcpck::launch_header_swap(h, num_cus, s) : e;
}

// hdr: RECEIVE's host-order headers to hdr[32k, 32k + 32) instead of in place;
// ps, pev: launch_patch_on.
hipError_t launch_fixed(tcpck_ctx *ctx, const Plan &p, int mode, uint8_t *arena, uint64_t stride, uint32_t len,
                        uint64_t count, void *out, uint8_t *hdr, hipStream_t s, const Hooks &hk, hipStream_t ps,
                        hipEvent_t pev) {
  const auto num_cus = static_cast<uint32_t>(ctx->num_cus);
  tcpck::PatchArgs pa{};
  pa.arena = arena;
  pa.stride = stride;
  pa.count = count;
  pa.sums = static_cast<uint16_t *>(out);
  pa.lo = 0;
  pa.hi = (count - 1) * stride + len;
  tcpck::HeaderArgs h{};
  h.arena = arena;
  h.stride = stride;
  h.count = count;
  h.out = hdr;
  h.store_bits = hk.hdr_store_bits;
  return launch_plan(p, pa, h, num_cus, s, hk, ps, pev, [&]() -> hipError_t {
    const int param = p.param;
    const uint32_t oversub = static_cast<uint32_t>(param >> 16) & 0xFFu;
    const uint32_t blocks_per_cu = static_cast<uint32_t>(param >> 8) & 0xFFu;
    if (p.kernel == TCPCK_KERNEL_RSTREAM) {
      tcpck::FixedStreamArgs a{};
      a.mode = mode == TCPCK_MODE_REF ? tcpck::kRef : tcpck::kRfc1071;
      a.arena = arena;
      a.stride = stride;
      a.count = count;
      a.order = 0xFFu;  // default block order (variants 14-19 choose an XCD order)
      a.out = out;
      a.dbg = static_cast<uint64_t *>(ctx->dbg);  // set by the probe library only
      a.blocks_per_cu = blocks_per_cu;
      a.oversub = oversub;
      a.defer_field = p.fill == Fill::kDeferred ? 1u : 0u;
      return tcpck::launch_rstream(p.op, param & 0xFF, a, num_cus, s);
    }
    if (p.kernel == TCPCK_KERNEL_GSTREAM) {
      tcpck::GroupStreamArgs a{};
      a.arena = arena;
      a.len = len;
      a.count = count;
      a.out = out;
      a.oversub = oversub;
      return tcpck::launch_gstream(p.op, param & 0xFFFF, a, num_cus, s);
    }
    if (p.kernel == TCPCK_KERNEL_SSTREAM || p.kernel == TCPCK_KERNEL_VVSTREAM) {
      tcpck::RunArgs a{};
      a.mode = mode == TCPCK_MODE_REF ? tcpck::kRef : tcpck::kRfc1071;
      a.arena = arena;
      a.stride = stride;
      a.len = len;
      a.count = count;
      a.out = out;
      a.oversub = oversub;
      if (p.kernel == TCPCK_KERNEL_SSTREAM) {
        if (count == 1) a.stride = (static_cast<uint64_t>(len) + 15) & ~uint64_t{15};  // one image: never read
        if (p.hdr == Hdr::kFused) a.hdr = hdr;
        return tcpck::launch_sstream(p.op, param & 0xFF, true, a, num_cus, s);
      }
      a.blocks_per_cu = blocks_per_cu;
      a.dbg = static_cast<uint64_t *>(ctx->dbg);  // set by the probe library only
      return tcpck::launch_vvstream(p.op, param & 0xFF, true, a, num_cus, s);
    }
    SegArgs a{};
    a.arena = arena;
    a.stride = stride;
    a.len = len;
    a.count = count;
    a.out = out;
    a.oversub = oversub;
    a.order = ((param >> 24) & 1u) ? 4u : 0xFFu;  // bit 24: XCD-chunked order, groups of 16 blocks
    a.rot = blocks_per_cu;  // bits 8-15: the W-wave shapes' rotation multiplier
    return tcpck::launch_seg(p.op, mode, true, static_cast<tcpck::SegShape>((param & 0xFF) - 1), a, num_cus, s);
  });
}

hipError_t launch_var(tcpck_ctx *ctx, const Plan &p, int mode, uint8_t *arena, const uint64_t *off,
                      const uint32_t *len, uint64_t base, uint64_t count, void *out, const tcpck_layout *layout,
                      uint8_t *hdr, hipStream_t s, const Hooks &hk, hipStream_t ps, hipEvent_t pev) {
  const auto num_cus = static_cast<uint32_t>(ctx->num_cus);
  tcpck::PatchArgs pa{};
  pa.arena = arena;
  pa.offsets = off;
  pa.lengths = len;
  pa.base = base;
  pa.count = count;
  pa.sums = static_cast<uint16_t *>(out);
  pa.packed = (p.fill == Fill::kUpdate && layout && (layout->flags & TCPCK_LAYOUT_PACKED)) ? 1u : 0u;
  tcpck::HeaderArgs h{};
  h.arena = arena;
  h.offsets = off;
  h.count = count;
  h.out = hdr;
  h.store_bits = hk.hdr_store_bits;
  return launch_plan(p, pa, h, num_cus, s, hk, ps, pev, [&]() -> hipError_t {
    const int param = p.param;
    const uint32_t oversub = static_cast<uint32_t>(param >> 16) & 0xFFu;
    if (p.kernel == TCPCK_KERNEL_SEG) {
      SegArgs a{};
      a.arena = arena;
      a.offsets = off;
      a.lengths = len;
      a.base = base;
      a.count = count;
      a.out = out;
      a.oversub = oversub;
      a.order = ((param >> 24) & 1u) ? 4u : 0xFFu;  // bit 24: XCD-chunked order, groups of 16 blocks
      return tcpck::launch_seg(p.op, mode, false, static_cast<tcpck::SegShape>((param & 0xFF) - 1), a, num_cus, s);
    }
    tcpck::RunArgs a{};
    a.mode = mode == TCPCK_MODE_REF ? tcpck::kRef : tcpck::kRfc1071;
    a.arena = arena;
    a.offsets = off;
    a.lengths = len;
    a.base = base;
    a.count = count;
    a.out = out;
    a.oversub = oversub;
    a.total_bytes = layout ? layout->total_bytes : 0;
    if (p.kernel == TCPCK_KERNEL_RVSTREAM) return tcpck::launch_rvstream(p.op, param & 0xFF, a, num_cus, s);
    if (p.kernel == TCPCK_KERNEL_SSTREAM) {
      if (p.hdr == Hdr::kFused) a.hdr = hdr;
      return tcpck::launch_sstream(p.op, param & 0xFF, false, a, num_cus, s);
    }
    a.blocks_per_cu = static_cast<uint32_t>(param >> 8) & 0xFFu;
    a.dbg = static_cast<uint64_t *>(ctx->dbg);  // set by the probe library only
    return tcpck::launch_vvstream(p.op, param & 0xFF, false, a, num_cus, s);
  });
}

// A sub-range of an offset-list batch keeps the flags and the length bounds,
// and its byte hint scales with its image count, so its typical image -- the
// quantity AUTO chooses by -- is the whole batch's and every chunk runs the
// same form (tcpck_tuning.h).
tcpck_layout sub_layout(const tcpck_layout &layout, uint64_t n, uint64_t count) {
  tcpck_layout sub = layout;
  sub.total_bytes = static_cast<uint64_t>(static_cast<unsigned __int128>(layout.total_bytes) * n / count);
  return sub;
}

// Patches bytes 28-29 of host images after a FILL computed on the device
// (the device filled its staging copy; the host image is the caller's).
void patch_fields(uint8_t *arena, uint64_t k0, uint64_t n, const uint16_t *res,
                  const uint64_t *off, const uint32_t *len, uint64_t stride, uint32_t flen) {
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t o = off ? off[k0 + k] : (k0 + k) * stride;
    const uint32_t l = len ? len[k0 + k] : flen;
    if (l >= 30) std::memcpy(arena + o + 28, &res[k], 2);
  }
}

}  // namespace

// ---- the router's entry points (tcpck_api_internal.h) -------------------------
namespace tcpck {
namespace api {

hipError_t run_fixed(tcpck_ctx *ctx, int op, int mode, uint8_t *arena, uint64_t stride, uint32_t len, uint64_t count,
                     void *out, int kernel, int param, hipStream_t s, uint8_t *hdr, const Hooks &hk) {
  const Plan plan = plan_fixed(op, mode, arena, stride, len, count, out != nullptr, hdr != nullptr, kernel, param, hk);
  return launch_fixed(ctx, plan, mode, arena, stride, len, count, out, hdr, s, hk, nullptr, nullptr);
}

hipError_t run_var(tcpck_ctx *ctx, int op, int mode, uint8_t *arena, const uint64_t *off, const uint32_t *len,
                   uint64_t base, uint64_t count, void *out, const tcpck_layout *layout, int kernel, int param,
                   hipStream_t s, uint8_t *hdr, const Hooks &hk) {
  if (op == TCPCK_OP_RECEIVE && base != 0) return hipErrorInvalidValue;  // device batches only
  const Plan plan = plan_var(op, mode, layout, count, out != nullptr, hdr != nullptr, kernel, param, hk);
  return launch_var(ctx, plan, mode, arena, off, len, base, count, out, layout, hdr, s, hk, nullptr, nullptr);
}

namespace {

// A scratch slot for one out-less FILL, its mutex held (nullptr: none, the
// caller runs the in-stream form).  None while `s` is under stream capture:
// a captured event record would order later uncaptured FILLs against a graph
// node, and a replayed graph would share the slot with no ordering at all.
tcpck_ctx::ScratchSlot *take_scratch(tcpck_ctx *ctx, hipStream_t s, std::unique_lock<std::mutex> &held) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (cs != hipStreamCaptureStatusNone) return nullptr;
  constexpr int n = tcpck_ctx::kScratchSlots;
  int pick = -1;
  {
    std::lock_guard<std::mutex> lk(ctx->scratch_mu);
    ++ctx->scratch_calls;
    if (!ctx->scratch[0].buf) {  // first use (or a retry after a refusal): every slot, or none
      if (ctx->scratch_calls < ctx->scratch_retry_at) return nullptr;
      for (auto &slot : ctx->scratch) {
        void *p = nullptr;
        hipEvent_t ev = nullptr;
        const bool forced = ctx->probe_scratch_fail > 0;  // probe library (tests): a refused allocation
        if (forced) --ctx->probe_scratch_fail;
        if (forced || hipMalloc(&p, tcpck::api::kScratchImages * 2) != hipSuccess ||
            hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
          if (p) (void)hipFree(p);
          (void)hipGetLastError();
          for (auto &sl : ctx->scratch) {
            if (sl.buf) (void)hipFree(sl.buf);
            if (sl.ev) (void)hipEventDestroy(sl.ev);
            sl.buf = nullptr;
            sl.ev = nullptr;
          }
          // not latched: the refusal may be transient (memory pressure, another
          // thread capturing a graph in global mode); this call and the next
          // kScratchRetry - 1 run the in-stream form, then allocation is retried
          ++ctx->scratch_refusals;
          ctx->scratch_retry_at = ctx->scratch_calls + tcpck::api::kScratchRetry;
          return nullptr;
        }
        slot.buf = static_cast<uint16_t *>(p);
        slot.ev = ev;
      }
      ctx->scratch_images = tcpck::api::kScratchImages;
    }
    // an idle slot (never used, or its last user's work done), else the next in turn
    for (int i = 0; i < n && pick < 0; ++i) {
      auto &slot = ctx->scratch[(ctx->scratch_next + i) % n];
      std::unique_lock<std::mutex> try_lk(slot.mu, std::try_to_lock);
      if (!try_lk.owns_lock()) continue;
      if (!slot.used || hipEventQuery(slot.ev) == hipSuccess) {
        pick = static_cast<int>((ctx->scratch_next + i) % n);
        held = std::move(try_lk);
      }
    }
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
    if (pick < 0) pick = static_cast<int>(ctx->scratch_next % n);
    ctx->scratch_next = static_cast<unsigned>(pick + 1);
  }
  // every slot busy: wait for the chosen one's holder with scratch_mu released,
  // so other callers can still take a slot that frees meanwhile
  if (!held.owns_lock()) held = std::unique_lock<std::mutex>(ctx->scratch[pick].mu);
  return &ctx->scratch[pick];
}

// launch(k0, n, results) for images [k0, k0 + n), n <= scratch_images, with
// the slot's previous use waited for first (always, not only when the stream
// differs -- a destroyed stream's handle can come back for a new stream while
// the old one's work still runs) and the slot's event recorded after.
template <typename Launch>
hipError_t with_scratch(tcpck_ctx *ctx, tcpck_ctx::ScratchSlot *slot, uint64_t count, hipStream_t s,
                        Launch launch) {
  hipError_t e = hipSuccess;
  if (slot->used) e = hipStreamWaitEvent(s, slot->ev, 0);
  for (uint64_t k0 = 0; k0 < count && e == hipSuccess; k0 += ctx->scratch_images)
    e = launch(k0, std::min(ctx->scratch_images, count - k0), slot->buf);
  const hipError_t er = hipEventRecord(slot->ev, s);
  if (er == hipSuccess) slot->used = true;
  return e != hipSuccess ? e : er;
}

// ---- pipelined FILL (round 6) --------------------------
// A FILL whose form has a field pass (the deferred-field forms and the update
// form: Plan::field_pass) runs the stream over all images and then the
// field pass over all images, one after the other.  Pipelined, the batch is cut
// into K chunks: chunk i's stream pass goes on the caller's stream, its field
// pass on the context's `pipe` stream after an event behind that stream pass,
// so the field pass of chunk i runs beside the stream pass of chunk i + 1, and
// the caller's stream waits for the last field pass (pipe_ev[K]) before
// anything it enqueues next.  Chunks are disjoint image ranges: a field pass
// writes only bytes 28-29 of its own chunk's images, which no other chunk's
// stream sums, and it reads only its own chunk's results.

constexpr int kFillPipeAuto = 0;          // AUTO's chunk count (0: not pipelined), DESIGN.md section 8
constexpr uint64_t kFillPipeMinImages = 4096;  // per chunk

hipError_t ensure_pipe(tcpck_ctx *ctx) {
  if (ctx->pipe) return hipSuccess;
  hipStream_t st = nullptr;
  hipError_t e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, ctx->pipe_prio);
  for (int i = 0; i <= tcpck_ctx::kPipeMax && e == hipSuccess; ++i)
    if (!ctx->pipe_ev[i]) e = hipEventCreateWithFlags(&ctx->pipe_ev[i], hipEventDisableTiming);
  if (e != hipSuccess) {  // the events made so far stay for the next attempt; freed by free_pipe
    if (st) (void)hipStreamDestroy(st);
    (void)hipGetLastError();
    return e;
  }
  ctx->pipe = st;
  return hipSuccess;
}

// K for this FILL (<= 1: not pipelined).  Only forms with a field pass, only
// with the caller's stream not capturing (the pipe stream would join the
// capture), and at least kFillPipeMinImages per chunk.
int fill_pipe_k(int kernel, bool has_field_pass, uint64_t count, hipStream_t s, const Hooks &hk) {
  if (kernel != TCPCK_KERNEL_AUTO || !has_field_pass) return 0;
  int k = hk.fill_pipe >= 0 ? hk.fill_pipe : kFillPipeAuto;
  k = static_cast<int>(std::min<uint64_t>(std::min(k, tcpck_ctx::kPipeMax), count / kFillPipeMinImages));
  if (k <= 1) return 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return cs == hipStreamCaptureStatusNone ? k : 0;
}

// launch(k0, n, ps, pev) enqueues images [k0, k0 + n): the stream pass on s,
// the field pass on ps after pev (ps == nullptr: everything on s).
// (one_stream, probe library: the same chunks with both passes on s -- the
// cost of chunking alone, without the second stream)
template <typename Launch>
hipError_t fill_pipelined(tcpck_ctx *ctx, int k, uint64_t count, hipStream_t s, bool one_stream, Launch launch) {
  std::lock_guard<std::mutex> lk(ctx->pipe_mu);
  if (ensure_pipe(ctx) != hipSuccess) return launch(0, count, nullptr, nullptr);  // the serial form
  hipError_t e = hipSuccess;
  const uint64_t per = (count + static_cast<uint64_t>(k) - 1) / static_cast<uint64_t>(k);
  int i = 0;
  for (uint64_t k0 = 0; k0 < count && e == hipSuccess; k0 += per, ++i)
    e = one_stream ? launch(k0, std::min(per, count - k0), nullptr, nullptr)
                   : launch(k0, std::min(per, count - k0), ctx->pipe, ctx->pipe_ev[i]);
  // join, also after an error: nothing the caller enqueues next may overtake a field pass already queued
  hipError_t ej = hipEventRecord(ctx->pipe_ev[tcpck_ctx::kPipeMax], ctx->pipe);
  if (ej == hipSuccess) ej = hipStreamWaitEvent(s, ctx->pipe_ev[tcpck_ctx::kPipeMax], 0);
  return e != hipSuccess ? e : ej;
}

// A FILL from its batch's plan, pipelined when fill_pipe_k says so.
hipError_t fill_fixed(tcpck_ctx *ctx, const Plan &plan, int mode, uint8_t *arena, uint64_t stride, uint32_t len,
                      uint64_t count, uint16_t *out, int kernel, int param, hipStream_t s, const Hooks &hk) {
  // images [k0, k0 + n) from the plan; a lone last image in a gapped layout has
  // no stride to speak of and is planned on its own, as one packed image
  auto chunk = [&](uint64_t k0, uint64_t n, hipStream_t ps, hipEvent_t pev) {
    uint8_t *at = arena + k0 * stride;
    if (n > 1 || stride == len) return launch_fixed(ctx, plan, mode, at, stride, len, n, out + k0, nullptr, s, hk, ps, pev);
    const Plan one = plan_fixed(TCPCK_OP_FILL, mode, at, len, len, 1, out != nullptr, false, kernel, param, hk);
    return launch_fixed(ctx, one, mode, at, len, len, 1, out + k0, nullptr, s, hk, ps, pev);
  };
  const int k = fill_pipe_k(kernel, plan.field_pass(), count, s, hk);
  return k <= 1 ? chunk(0, count, nullptr, nullptr) : fill_pipelined(ctx, k, count, s, hk.pipe_one_stream, chunk);
}

hipError_t fill_var(tcpck_ctx *ctx, const Plan &plan, int mode, uint8_t *arena, const uint64_t *off,
                    const uint32_t *len, uint64_t count, uint16_t *out, const tcpck_layout *layout, int kernel,
                    hipStream_t s, const Hooks &hk) {
  auto chunk = [&](uint64_t k0, uint64_t n, hipStream_t ps, hipEvent_t pev) {
    tcpck_layout sub{};
    if (layout) sub = sub_layout(*layout, n, count);
    return launch_var(ctx, plan, mode, arena, off + k0, len + k0, 0, n, out + k0, layout ? &sub : nullptr, nullptr, s,
                      hk, ps, pev);
  };
  const int k = fill_pipe_k(kernel, plan.field_pass(), count, s, hk);
  return k <= 1 ? chunk(0, count, nullptr, nullptr) : fill_pipelined(ctx, k, count, s, hk.pipe_one_stream, chunk);
}

}  // namespace

int batch_fixed_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, uint64_t stride, uint32_t len, uint64_t count,
                   void *d_out, int kernel, int param, hipStream_t s, const Hooks &hk) {
  if (!ctx || !valid_device_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  // images start at even addresses: the kernels pair bytes into u16 words by address
  if (!d_arena || (reinterpret_cast<uintptr_t>(d_arena) & 1) || (len & 1) || (stride & 1) ||
      (count > 1 && stride < len))
    return TCPCK_EINVAL;
  if (!d_out && op != TCPCK_OP_FILL) return TCPCK_EINVAL;
  if (op == TCPCK_OP_FILL && len < 30) return TCPCK_EINVAL;
  if (op == TCPCK_OP_RECEIVE && len < TCPCK_HEADER_BYTES) return TCPCK_EINVAL;
  if (count > 1 && stride > (UINT64_MAX - len) / (count - 1)) return TCPCK_EINVAL;
  if (count == 1) stride = len;  // one image: its stride is never read; the run kernels assume stride >= len
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  auto *arena = static_cast<uint8_t *>(d_arena);
  if (op != TCPCK_OP_FILL)
    return hip_status(run_fixed(ctx, op, mode, arena, stride, len, count, d_out, kernel, param, s, nullptr, hk));
  // FILL without a results buffer under AUTO (the reference's call shape,
  // socket-manager.cc:9-10): when AUTO's form for the layout has a field pass,
  // which reads the results back -- rstream's and vvstream's deferred fields,
  // the update pass (C2 in-stream 69.3 % -> 76-77 %, C3 53.7 -> 62 %,
  // profiles/r03/fill_forms.log) -- the batch is planned as with a results
  // buffer and the results go to a ctx scratch slot; every other form (gstream,
  // seg, the in-stream run forms) launches with out = NULL and takes no slot.
  auto *out = static_cast<uint16_t *>(d_out);
  const bool scratch = !out && kernel == TCPCK_KERNEL_AUTO;
  Plan plan = plan_fixed(op, mode, arena, stride, len, count, out || scratch, false, kernel, param, hk);
  if (scratch && plan.field_pass()) {
    std::unique_lock<std::mutex> held;
    if (auto *slot = take_scratch(ctx, s, held))
      return hip_status(with_scratch(ctx, slot, count, s, [&](uint64_t k0, uint64_t n, uint16_t *res) {
        return fill_fixed(ctx, plan, mode, arena + k0 * stride, stride, len, n, res, kernel, param, s, hk);
      }));
    plan = plan_fixed(op, mode, arena, stride, len, count, false, false, kernel, param, hk);  // no slot: in-stream
  }
  return hip_status(fill_fixed(ctx, plan, mode, arena, stride, len, count, out, kernel, param, s, hk));
}

int batch_var_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, const uint64_t *d_offsets,
                 const uint32_t *d_lengths, uint64_t count, void *d_out, const tcpck_layout *layout, int kernel,
                 int param, hipStream_t s, const Hooks &hk) {
  if (!ctx || !valid_device_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || !d_offsets || !d_lengths || (reinterpret_cast<uintptr_t>(d_arena) & 1)) return TCPCK_EINVAL;
  if (!d_out && op != TCPCK_OP_FILL) return TCPCK_EINVAL;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  auto *arena = static_cast<uint8_t *>(d_arena);
  if (op != TCPCK_OP_FILL)
    return hip_status(run_var(ctx, op, mode, arena, d_offsets, d_lengths, 0, count, d_out, layout, kernel, param, s,
                              nullptr, hk));
  auto *out = static_cast<uint16_t *>(d_out);
  const bool scratch = !out && kernel == TCPCK_KERNEL_AUTO;  // (as batch_fixed_ex)
  Plan plan = plan_var(op, mode, layout, count, out || scratch, false, kernel, param, hk);
  if (scratch && plan.field_pass()) {
    std::unique_lock<std::mutex> held;
    if (auto *slot = take_scratch(ctx, s, held))
      return hip_status(with_scratch(ctx, slot, count, s, [&](uint64_t k0, uint64_t n, uint16_t *res) {
        tcpck_layout sub{};
        if (layout) sub = sub_layout(*layout, n, count);
        return fill_var(ctx, plan, mode, arena, d_offsets + k0, d_lengths + k0, n, res, layout ? &sub : nullptr,
                        kernel, s, hk);
      }));
    plan = plan_var(op, mode, layout, count, false, false, kernel, param, hk);  // no slot: in-stream
  }
  return hip_status(fill_var(ctx, plan, mode, arena, d_offsets, d_lengths, count, out, layout, kernel, s, hk));
}

int check_receive(const tcpck_ctx *ctx, int mode, const void *d_arena, uint64_t &stride, uint32_t len,
                  const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, const uint8_t *d_ok,
                  const void *d_hdr) {
  if (!ctx || !valid_device_op_mode(TCPCK_OP_VERIFY, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || !d_ok || (reinterpret_cast<uintptr_t>(d_arena) & 1) || (reinterpret_cast<uintptr_t>(d_hdr) & 3))
    return TCPCK_EINVAL;
  if (count > (UINT64_MAX >> 6)) return TCPCK_EINVAL;
  if (!d_offsets) {
    if ((len & 1) || (stride & 1) || len < TCPCK_HEADER_BYTES || (count > 1 && stride < len)) return TCPCK_EINVAL;
    if (count > 1 && stride > (UINT64_MAX - len) / (count - 1)) return TCPCK_EINVAL;
    if (count == 1) stride = len;
  } else if (!d_lengths) {
    return TCPCK_EINVAL;
  }
  return TCPCK_OK;
}

int batch_receive_ex(tcpck_ctx *ctx, int mode, void *d_arena, uint64_t stride, uint32_t len,
                     const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, uint8_t *d_ok,
                     void *d_hdr, const tcpck_layout *layout, int kernel, int param, hipStream_t s,
                     const Hooks &hk) {
  if (!d_hdr) {  // TCPCK_OP_RECEIVE: the headers converted in place
    return d_offsets ? batch_var_ex(ctx, TCPCK_OP_RECEIVE, mode, d_arena, d_offsets, d_lengths, count, d_ok, layout,
                                    kernel, param, s, hk)
                     : batch_fixed_ex(ctx, TCPCK_OP_RECEIVE, mode, d_arena, stride, len, count, d_ok, kernel, param,
                                      s, hk);
  }
  const int rc = check_receive(ctx, mode, d_arena, stride, len, d_offsets, d_lengths, count, d_ok, d_hdr);
  if (rc != TCPCK_OK || count == 0) return rc;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  auto *arena = static_cast<uint8_t *>(d_arena);
  auto *hdr = static_cast<uint8_t *>(d_hdr);
  return hip_status(d_offsets ? run_var(ctx, TCPCK_OP_RECEIVE, mode, arena, d_offsets, d_lengths, 0, count, d_ok,
                                        layout, kernel, param, s, hdr, hk)
                              : run_fixed(ctx, TCPCK_OP_RECEIVE, mode, arena, stride, len, count, d_ok, kernel,
                                          param, s, hdr, hk));
}

}  // namespace api
}  // namespace tcpck

// helpers of tcpck_host_batch_*_multi
namespace {

// Runs shard i of n as job(i) -- shards 1.. on their own threads, shard 0 on the
// caller's -- and returns the first nonzero status in shard order.
template <typename Job>
int run_shards(int n, Job job_raw) {
  // nothing may escape a shard's thread (std::terminate) or the C ABI
  auto job = [&job_raw](int i) -> int {
    try {
      return job_raw(i);
    } catch (const std::bad_alloc &) {
      return TCPCK_ENOMEM;
    } catch (...) {
      return TCPCK_EINVAL;
    }
  };
  std::vector<int> rc;
  std::vector<std::thread> th;
  try {
    rc.assign(static_cast<size_t>(n), TCPCK_OK);
    th.reserve(static_cast<size_t>(n));
  } catch (...) {
    return TCPCK_ENOMEM;
  }
  for (int i = 1; i < n; ++i) {
    try {
      th.emplace_back([&rc, &job, i] { rc[static_cast<size_t>(i)] = job(i); });
    } catch (...) {  // no thread: run it here
      rc[static_cast<size_t>(i)] = job(i);
    }
  }
  rc[0] = job(0);
  for (auto &t : th) t.join();
  for (int r : rc)
    if (r != TCPCK_OK) return r;
  return TCPCK_OK;
}

bool valid_ctx_list(tcpck_ctx *const *ctxs, int n_ctx) {
  if (!ctxs || n_ctx < 1) return false;
  for (int i = 0; i < n_ctx; ++i)
    if (!ctxs[i]) return false;
  return true;
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
  // (the results scratch of out-less FILLs is allocated on first use: take_scratch)
  *out = ctx;
  return TCPCK_OK;
}

int tcpck_ctx_destroy(tcpck_ctx *ctx) {
  if (!ctx) return TCPCK_EINVAL;
  {
    DeviceGuard g(ctx->device);
    free_stage(ctx);
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
// tuning entry points: tcpck_ex.hip, and tcpck_ex_probe.hip in the probe library)

// ---- batched retransmit: ACK rewrite + incremental update ----------------------
int tcpck_batch_set_ack(tcpck_ctx *ctx, int mode, void *d_arena, const uint64_t *d_offsets, uint64_t stride,
                        uint64_t count, const uint32_t *d_acks, uint32_t ack, uint16_t *d_out,
                        tcpck_stream stream) {
  if (!ctx || (mode != TCPCK_MODE_REF && mode != TCPCK_MODE_RFC1071)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || (reinterpret_cast<uintptr_t>(d_arena) & 1)) return TCPCK_EINVAL;
  if (!d_offsets) {
    if ((stride & 1) || (count > 1 && stride < 30)) return TCPCK_EINVAL;
    if (count > 1 && stride > (UINT64_MAX - 30) / (count - 1)) return TCPCK_EINVAL;
  }
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::AckArgs a{};
  a.arena = static_cast<uint8_t *>(d_arena);
  a.offsets = d_offsets;
  a.stride = stride;
  a.count = count;
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
  if (!d_offsets) {
    if ((stride & 1) || (count > 1 && stride < TCPCK_HEADER_BYTES)) return TCPCK_EINVAL;
    if (count > 1 && stride > (UINT64_MAX - TCPCK_HEADER_BYTES) / (count - 1)) return TCPCK_EINVAL;
  }
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::HeaderArgs a{};
  a.arena = static_cast<uint8_t *>(d_arena);
  a.offsets = d_offsets;
  a.stride = stride;
  a.count = count;
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

// ---- batched, host memory: chunked H2D -> kernel -> D2H on two streams ---------
int tcpck_host_batch_fixed(tcpck_ctx *ctx, int op, int mode, void *h_arena, uint64_t stride,
                           uint32_t len, uint64_t count, void *h_out) {
  if (!ctx || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || (len & 1) || (stride & 1) || (count > 1 && stride < len)) return TCPCK_EINVAL;
  if (!h_out && op != TCPCK_OP_FILL) return TCPCK_EINVAL;
  if (op == TCPCK_OP_FILL && len < 30) return TCPCK_EINVAL;
  if (count > 1 && stride > (UINT64_MAX - len) / (count - 1)) return TCPCK_EINVAL;
  if (count == 1) stride = len;
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  const uint64_t step = std::max<uint64_t>(stride, 2);
  const uint64_t per = std::max<uint64_t>(1, ctx->chunk_bytes / step);
  const uint64_t chunk_imgs = std::min(per, count);
  int rc = ensure_stage(ctx, (chunk_imgs - 1) * stride + len, chunk_imgs);
  if (rc) return rc;
  std::vector<uint16_t> fill_res;
  if (op == TCPCK_OP_FILL && !h_out) fill_res.resize(count);
  auto *arena = static_cast<uint8_t *>(h_arena);
  auto *out_bytes = h_out ? static_cast<uint8_t *>(h_out) : reinterpret_cast<uint8_t *>(fill_res.data());
  const size_t es = out_elem(op);
  hipError_t e = hipSuccess;
  uint64_t c = 0;
  for (uint64_t k0 = 0; k0 < count && e == hipSuccess; k0 += chunk_imgs, ++c) {
    const int slot = static_cast<int>(c & 1);
    const uint64_t n = std::min(chunk_imgs, count - k0);
    const uint64_t bytes = (n - 1) * stride + len;
    hipStream_t s = ctx->s[slot];
    e = hipMemcpyAsync(ctx->stage[slot], arena + k0 * stride, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) break;
    e = tcpck::api::run_fixed(ctx, op, mode, ctx->stage[slot], stride, len, n, ctx->stage_out[slot],
                              TCPCK_KERNEL_AUTO, 0, s, nullptr, Hooks{});
    if (e != hipSuccess) break;
    e = hipMemcpyAsync(out_bytes + k0 * es, ctx->stage_out[slot], n * es, hipMemcpyDeviceToHost, s);
  }
  for (int i = 0; i < 2; ++i) {
    hipError_t e2 = hipStreamSynchronize(ctx->s[i]);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return hip_status(e);
  if (op == TCPCK_OP_FILL)
    patch_fields(arena, 0, count, reinterpret_cast<const uint16_t *>(out_bytes), nullptr, nullptr,
                 stride, len);
  return TCPCK_OK;
}

int tcpck_host_batch_var(tcpck_ctx *ctx, int op, int mode, void *h_arena, const uint64_t *h_offsets,
                         const uint32_t *h_lengths, uint64_t count, void *h_out) {
  if (!ctx || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || !h_offsets || !h_lengths) return TCPCK_EINVAL;
  if (!h_out && op != TCPCK_OP_FILL) return TCPCK_EINVAL;
  uint64_t max_len = 0, min_len = UINT64_MAX;
  bool packed = true, sorted = true;
  for (uint64_t k = 0; k < count; ++k) {
    if ((h_offsets[k] | h_lengths[k]) & 1) return TCPCK_EINVAL;
    if (op == TCPCK_OP_FILL && h_lengths[k] < 30) return TCPCK_EINVAL;
    max_len = std::max<uint64_t>(max_len, h_lengths[k]);
    min_len = std::min<uint64_t>(min_len, h_lengths[k]);
    if (k + 1 < count && h_offsets[k] + h_lengths[k] != h_offsets[k + 1]) packed = false;
    if (k + 1 < count && h_offsets[k] + h_lengths[k] > h_offsets[k + 1]) sorted = false;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  const uint64_t cap = std::max<uint64_t>(ctx->chunk_bytes, max_len + 16);
  const uint64_t max_imgs = std::min<uint64_t>(count, std::max<uint64_t>(cap / 32, 1));
  int rc = ensure_stage(ctx, cap, max_imgs);
  if (rc) return rc;
  std::vector<uint16_t> fill_res;
  if (op == TCPCK_OP_FILL && !h_out) fill_res.resize(count);
  auto *arena = static_cast<uint8_t *>(h_arena);
  auto *out_bytes = h_out ? static_cast<uint8_t *>(h_out) : reinterpret_cast<uint8_t *>(fill_res.data());
  const size_t es = out_elem(op);
  tcpck_layout lay{};
  lay.min_len = static_cast<uint32_t>(std::min<uint64_t>(min_len, UINT32_MAX));
  lay.max_len = static_cast<uint32_t>(std::min<uint64_t>(max_len, UINT32_MAX));
  lay.flags = (packed ? TCPCK_LAYOUT_PACKED : 0u) | (sorted ? TCPCK_LAYOUT_SORTED : 0u);
  hipError_t e = hipSuccess;
  uint64_t c = 0;
  for (uint64_t k0 = 0; k0 < count && e == hipSuccess; ++c) {
    // greedy chunk: extend while the hull [lo, hi) of the chunk fits the stage
    uint64_t lo = h_offsets[k0] & ~uint64_t{15}, hi = h_offsets[k0] + h_lengths[k0];
    uint64_t k1 = k0 + 1, chunk_bytes = h_lengths[k0];
    while (k1 < count && k1 - k0 < max_imgs) {
      const uint64_t nlo = std::min(lo, h_offsets[k1] & ~uint64_t{15});
      const uint64_t nhi = std::max(hi, h_offsets[k1] + h_lengths[k1]);
      if (nhi - nlo > cap) break;
      lo = nlo;
      hi = nhi;
      chunk_bytes += h_lengths[k1];
      ++k1;
    }
    lay.total_bytes = chunk_bytes;  // the kernel policy sizes its grid by this launch's bytes
    const uint64_t n = k1 - k0;
    const int slot = static_cast<int>(c & 1);
    hipStream_t s = ctx->s[slot];
    e = hipMemcpyAsync(ctx->stage[slot], arena + lo, hi - lo, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ctx->stage_off[slot], h_offsets + k0, n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ctx->stage_len[slot], h_lengths + k0, n * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) break;
    e = tcpck::api::run_var(ctx, op, mode, ctx->stage[slot], ctx->stage_off[slot], ctx->stage_len[slot], lo, n,
                            ctx->stage_out[slot], &lay, TCPCK_KERNEL_AUTO, 0, s, nullptr, Hooks{});
    if (e != hipSuccess) break;
    e = hipMemcpyAsync(out_bytes + k0 * es, ctx->stage_out[slot], n * es, hipMemcpyDeviceToHost, s);
    k0 = k1;
  }
  for (int i = 0; i < 2; ++i) {
    hipError_t e2 = hipStreamSynchronize(ctx->s[i]);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return hip_status(e);
  if (op == TCPCK_OP_FILL)
    patch_fields(arena, 0, count, reinterpret_cast<const uint16_t *>(out_bytes), h_offsets, h_lengths,
                 0, 0);
  return TCPCK_OK;
}

// ---- host batches over several contexts (one per GPU) ---------------------------

int tcpck_host_batch_fixed_multi(tcpck_ctx *const *ctxs, int n_ctx, int op, int mode, void *h_arena,
                                 uint64_t stride, uint32_t len, uint64_t count, void *h_out) {
  if (!valid_ctx_list(ctxs, n_ctx) || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || (!h_out && op != TCPCK_OP_FILL)) return TCPCK_EINVAL;
  if (count > 1 && stride > (UINT64_MAX - len) / (count - 1)) return TCPCK_EINVAL;
  const uint64_t n = std::min<uint64_t>(static_cast<uint64_t>(n_ctx), count);
  const size_t es = out_elem(op);
  auto *arena = static_cast<uint8_t *>(h_arena);
  auto *out = static_cast<uint8_t *>(h_out);
  return run_shards(static_cast<int>(n), [&](int i) {
    const uint64_t q = count / n, r = count % n, ui = static_cast<uint64_t>(i);
    const uint64_t k0 = ui * q + std::min(ui, r), k1 = k0 + q + (ui < r ? 1 : 0);
    return tcpck_host_batch_fixed(ctxs[i], op, mode, arena + k0 * stride, stride, len, k1 - k0,
                                  out ? out + k0 * es : nullptr);
  });
}

int tcpck_host_batch_var_multi(tcpck_ctx *const *ctxs, int n_ctx, int op, int mode, void *h_arena,
                               const uint64_t *h_offsets, const uint32_t *h_lengths, uint64_t count,
                               void *h_out) {
  if (!valid_ctx_list(ctxs, n_ctx) || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || !h_offsets || !h_lengths || (!h_out && op != TCPCK_OP_FILL)) return TCPCK_EINVAL;
  const uint64_t n = std::min<uint64_t>(static_cast<uint64_t>(n_ctx), count);
  // shard starts balanced by bytes: shard i begins at the first image whose
  // byte prefix reaches i/n of the total (a 1492-B image is 15.5x a 96-B one)
  uint64_t total = 0;
  for (uint64_t k = 0; k < count; ++k) total += h_lengths[k];
  std::vector<uint64_t> cut;
  try {
    cut.assign(n + 1, count);
  } catch (...) {
    return TCPCK_ENOMEM;
  }
  cut[0] = 0;
  uint64_t pre = 0, k = 0;
  for (uint64_t i = 1; i < n; ++i) {
    const uint64_t target = static_cast<uint64_t>((static_cast<unsigned __int128>(total) * i) / n);
    while (k < count && pre < target) pre += h_lengths[k++];
    cut[i] = std::max(k, cut[i - 1]);
  }
  const size_t es = out_elem(op);
  auto *out = static_cast<uint8_t *>(h_out);
  return run_shards(static_cast<int>(n), [&](int i) {
    const uint64_t k0 = cut[static_cast<size_t>(i)], k1 = cut[static_cast<size_t>(i) + 1];
    if (k1 <= k0) return TCPCK_OK;
    return tcpck_host_batch_var(ctxs[i], op, mode, h_arena, h_offsets + k0, h_lengths + k0, k1 - k0,
                                out ? out + k0 * es : nullptr);
  });
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
