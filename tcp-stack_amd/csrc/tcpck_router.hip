// tcpck_router.hip -- the batch router: plan, then launch.
//
// tcpck_plan.h decides a batch once -- AUTO's kernel and param, FILL's and
// RECEIVE's form, whether the request is rejected (plan_fixed / plan_var; the
// policy and its measurements are in tcpck_plan.cc); the functions here launch
// a plan on the caller's buffers and decide nothing.  The images of a batch are
// one value, Images (tcpck_api_internal.h), whichever layout they have, so
// the launcher, the FILL front (scratch slots, the pipelined form) and the
// validated entry points exist once; its ImageSpan (tcpck_internal.h) is what
// every launcher's argument struct takes, assigned whole.
// tests/cpp/router_trace.cc records every launch of this file without a GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "tcpck.h"
#include "tcpck_tuning.h"
#include "tcpck_internal.h"
#include "tcpck_api_internal.h"

namespace tcpck {
namespace api {
namespace {

// device batches also take RECEIVE (VERIFY + TcpHeaderN2H)
bool valid_device_op_mode(int op, int mode) { return valid_op_mode(op == TCPCK_OP_RECEIVE ? TCPCK_OP_VERIFY : op, mode); }

// The plan of a whole batch, or of a lone image (Images::sub); a sub-range of
// an offset list launches from its batch's plan and is never planned itself.
Plan plan_for(int op, int mode, const Images &im, bool has_out, bool has_hdr, int kernel, int param, const Hooks &hk) {
  if (im.is_fixed()) return plan_fixed(op, mode, im.arena, im.stride, im.len, im.count, has_out, has_hdr, kernel, param, hk);
  return plan_var(op, mode, im.layout, im.count, has_out, has_hdr, kernel, param, hk);
}

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

// A plan's stream kernel on the batch.  Each launcher's argument struct gets
// the batch's span (the fields of its layout and zeros for the other layout's);
// rstream and gstream take fixed layouts only, rvstream offset lists only (the
// plans reject the rest).
hipError_t launch_stream(tcpck_ctx *ctx, const Plan &p, int mode, const Images &im, void *out, uint8_t *hdr,
                         hipStream_t s) {
  const auto num_cus = static_cast<uint32_t>(ctx->num_cus);
  const bool fixed = im.is_fixed();
  const int param = p.param;
  const uint32_t oversub = static_cast<uint32_t>(param >> 16) & 0xFFu;
  const uint32_t blocks_per_cu = static_cast<uint32_t>(param >> 8) & 0xFFu;
  switch (p.kernel) {
    case TCPCK_KERNEL_RSTREAM: {
      tcpck::FixedStreamArgs a{};
      a.mode = mode == TCPCK_MODE_REF ? tcpck::kRef : tcpck::kRfc1071;
      a.arena = im.arena;
      a.stride = im.stride;
      a.count = im.count;
      a.order = 0xFFu;  // default block order (variants 14-19 choose an XCD order)
      a.out = out;
      a.dbg = static_cast<uint64_t *>(ctx->dbg);  // set by the probe library only
      a.blocks_per_cu = blocks_per_cu;
      a.oversub = oversub;
      a.defer_field = p.fill == Fill::kDeferred ? 1u : 0u;
      return tcpck::launch_rstream(p.op, param & 0xFF, a, num_cus, s);
    }
    case TCPCK_KERNEL_GSTREAM: {
      tcpck::GroupStreamArgs a{};
      a.arena = im.arena;
      a.len = im.len;
      a.count = im.count;
      a.out = out;
      a.oversub = oversub;
      return tcpck::launch_gstream(p.op, param & 0xFFFF, a, num_cus, s);
    }
    case TCPCK_KERNEL_SEG: {
      tcpck::SegArgs a{};
      a.im = im;
      a.out = out;
      a.oversub = oversub;
      a.order = ((param >> 24) & 1u) ? 4u : 0xFFu;  // bit 24: XCD-chunked order, groups of 16 blocks
      if (fixed) a.rot = blocks_per_cu;  // bits 8-15: the W-wave shapes' rotation multiplier
      return tcpck::launch_seg(p.op, mode, fixed, static_cast<tcpck::SegShape>((param & 0xFF) - 1), a, num_cus, s);
    }
    case TCPCK_KERNEL_RVSTREAM:
    case TCPCK_KERNEL_SSTREAM:
    case TCPCK_KERNEL_VVSTREAM: {
      tcpck::RunArgs a{};
      a.mode = mode == TCPCK_MODE_REF ? tcpck::kRef : tcpck::kRfc1071;
      a.im = im;
      a.out = out;
      a.oversub = oversub;
      a.total_bytes = im.total_bytes;
      if (p.kernel == TCPCK_KERNEL_RVSTREAM) return tcpck::launch_rvstream(p.op, param & 0xFF, a, num_cus, s);
      if (p.kernel == TCPCK_KERNEL_SSTREAM) {
        if (fixed && im.count == 1) a.im.stride = (static_cast<uint64_t>(im.len) + 15) & ~uint64_t{15};  // one image: never read
        if (p.hdr == Hdr::kFused) a.hdr = hdr;
        return tcpck::launch_sstream(p.op, param & 0xFF, fixed, a, num_cus, s);
      }
      a.blocks_per_cu = blocks_per_cu;
      a.dbg = static_cast<uint64_t *>(ctx->dbg);  // set by the probe library only
      return tcpck::launch_vvstream(p.op, param & 0xFF, fixed, a, num_cus, s);
    }
    default: return hipErrorInvalidValue;  // (no plan that is not rejected names another kernel)
  }
}

// A plan's launches on the batch, in the plan's order: the header pass first,
// the stream kernel, then the field pass or the header pass after.
// hdr: RECEIVE's host-order headers to hdr[32k, 32k + 32) instead of in place;
// ps, pev: launch_patch_on.
hipError_t launch(tcpck_ctx *ctx, const Plan &p, int mode, const Images &im, void *out, uint8_t *hdr, hipStream_t s,
                  const Hooks &hk, hipStream_t ps, hipEvent_t pev) {
  const auto num_cus = static_cast<uint32_t>(ctx->num_cus);
  auto header_pass = [&]() {
    tcpck::HeaderArgs h{};
    h.im = im;
    h.out = hdr;
    h.store_bits = hk.hdr_store_bits;
    return tcpck::launch_header_swap(h, num_cus, s);
  };
  hipError_t e = p.hdr == Hdr::kFirst ? header_pass() : hipSuccess;
  if (e == hipSuccess) e = p.rejected ? hipErrorInvalidValue : launch_stream(ctx, p, mode, im, out, hdr, s);
  if (e != hipSuccess) return e;
  if (p.field_pass()) {  // the fields the stream left: write-through 2-B stores (launch_patch_fields)
    tcpck::PatchArgs pa{};
    pa.im = im;
    pa.sums = static_cast<uint16_t *>(out);
    if (im.is_fixed())
      pa.hi = (im.count - 1) * im.stride + im.len;  // (lo = 0)
    else
      pa.packed = (p.fill == Fill::kUpdate && im.layout && (im.layout->flags & TCPCK_LAYOUT_PACKED)) ? 1u : 0u;
    pa.update = p.fill == Fill::kUpdate ? 1u : 0u;
    pa.reverse = hk.patch_reverse ? 1u : 0u;
    return launch_patch_on(pa, num_cus, s, ps, pev);
  }
  return p.hdr == Hdr::kAfter ? header_pass() : e;
}

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
  if (e != hipSuccess) {  // the events made so far stay for the next attempt; freed with the context
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

}  // namespace

// ---- the router's entry points (tcpck_api_internal.h) -------------------------

hipError_t run(tcpck_ctx *ctx, int op, int mode, const Images &im, void *out, int kernel, int param, hipStream_t s,
               uint8_t *hdr, const Hooks &hk) {
  if (op == TCPCK_OP_RECEIVE && im.base != 0) return hipErrorInvalidValue;  // device batches only
  const Plan plan = plan_for(op, mode, im, out != nullptr, hdr != nullptr, kernel, param, hk);
  return launch(ctx, plan, mode, im, out, hdr, s, hk, nullptr, nullptr);
}

// A FILL from its batch's plan, pipelined when fill_pipe_k says so.
hipError_t fill(tcpck_ctx *ctx, const Plan &plan, int mode, const Images &im, uint16_t *out, int kernel, int param,
                hipStream_t s, const Hooks &hk) {
  // images [k0, k0 + n) from the plan; a lone image of a gapped layout from a plan of its own (Images::sub)
  auto chunk = [&](uint64_t k0, uint64_t n, hipStream_t ps, hipEvent_t pev) {
    const Images part = im.sub(k0, n);
    if (!part.lone) return launch(ctx, plan, mode, part, out + k0, nullptr, s, hk, ps, pev);
    const Plan one = plan_for(TCPCK_OP_FILL, mode, part, out != nullptr, false, kernel, param, hk);
    return launch(ctx, one, mode, part, out + k0, nullptr, s, hk, ps, pev);
  };
  const int k = fill_pipe_k(kernel, plan.field_pass(), im.count, s, hk);
  return k <= 1 ? chunk(0, im.count, nullptr, nullptr) : fill_pipelined(ctx, k, im.count, s, hk.pipe_one_stream, chunk);
}

namespace {

// A validated device batch (batch_fixed_ex / batch_var_ex).
int batch(tcpck_ctx *ctx, int op, int mode, const Images &im, void *d_out, int kernel, int param, hipStream_t s,
          const Hooks &hk) {
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  if (op != TCPCK_OP_FILL) return hip_status(run(ctx, op, mode, im, d_out, kernel, param, s, nullptr, hk));
  // FILL without a results buffer under AUTO (the reference's call shape,
  // socket-manager.cc:9-10): when AUTO's form for the layout has a field pass,
  // which reads the results back -- rstream's and vvstream's deferred fields,
  // the update pass (C2 in-stream 69.3 % -> 76-77 %, C3 53.7 -> 62 %,
  // profiles/r03/fill_forms.log) -- the batch is planned as with a results
  // buffer and the results go to a ctx scratch slot; every other form (gstream,
  // seg, the in-stream run forms) launches with out = NULL and takes no slot.
  auto *out = static_cast<uint16_t *>(d_out);
  const bool scratch = !out && kernel == TCPCK_KERNEL_AUTO;
  Plan plan = plan_for(op, mode, im, out || scratch, false, kernel, param, hk);
  if (scratch && plan.field_pass()) {
    std::unique_lock<std::mutex> held;
    if (auto *slot = take_scratch(ctx, s, held))
      return hip_status(with_scratch(ctx, slot, im.count, s, [&](uint64_t k0, uint64_t n, uint16_t *res) {
        return fill(ctx, plan, mode, im.sub(k0, n), res, kernel, param, s, hk);
      }));
    plan = plan_for(op, mode, im, false, false, kernel, param, hk);  // no slot: in-stream
  }
  return hip_status(fill(ctx, plan, mode, im, out, kernel, param, s, hk));
}

}  // namespace

int batch_fixed_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, uint64_t stride, uint32_t len, uint64_t count,
                   void *d_out, int kernel, int param, hipStream_t s, const Hooks &hk) {
  if (!ctx || !valid_device_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  // images start at even addresses: the kernels pair bytes into u16 words by address
  if (!d_arena || (reinterpret_cast<uintptr_t>(d_arena) & 1) || (!d_out && op != TCPCK_OP_FILL)) return TCPCK_EINVAL;
  const uint32_t min_len = op == TCPCK_OP_FILL ? 30 : (op == TCPCK_OP_RECEIVE ? TCPCK_HEADER_BYTES : 0);
  if (!valid_fixed(stride, len, count, min_len)) return TCPCK_EINVAL;
  return batch(ctx, op, mode, Images::fixed(static_cast<uint8_t *>(d_arena), stride, len, count), d_out, kernel, param,
               s, hk);
}

int batch_var_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, const uint64_t *d_offsets,
                 const uint32_t *d_lengths, uint64_t count, void *d_out, const tcpck_layout *layout, int kernel,
                 int param, hipStream_t s, const Hooks &hk) {
  if (!ctx || !valid_device_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || !d_offsets || !d_lengths || (reinterpret_cast<uintptr_t>(d_arena) & 1)) return TCPCK_EINVAL;
  if (!d_out && op != TCPCK_OP_FILL) return TCPCK_EINVAL;
  return batch(ctx, op, mode, Images::list(static_cast<uint8_t *>(d_arena), d_offsets, d_lengths, 0, count, layout),
               d_out, kernel, param, s, hk);
}

int check_receive(const tcpck_ctx *ctx, int mode, const void *d_arena, uint64_t &stride, uint32_t len,
                  const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, const uint8_t *d_ok,
                  const void *d_hdr) {
  if (!ctx || !valid_device_op_mode(TCPCK_OP_VERIFY, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || !d_ok || (reinterpret_cast<uintptr_t>(d_arena) & 1) || (reinterpret_cast<uintptr_t>(d_hdr) & 3))
    return TCPCK_EINVAL;
  if (count > (UINT64_MAX >> 6)) return TCPCK_EINVAL;
  if (d_offsets ? !d_lengths : !valid_fixed(stride, len, count, TCPCK_HEADER_BYTES)) return TCPCK_EINVAL;
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
  const Images im = d_offsets ? Images::list(arena, d_offsets, d_lengths, 0, count, layout)
                              : Images::fixed(arena, stride, len, count);
  return hip_status(run(ctx, TCPCK_OP_RECEIVE, mode, im, d_ok, kernel, param, s, static_cast<uint8_t *>(d_hdr), hk));
}

}  // namespace api
}  // namespace tcpck
