// tcpck_api_internal.h -- the context and the batch router shared by the C-ABI
// layer (tcpck_api.hip, tcpck_host_batch.hip), the router itself
// (tcpck_router.hip), its tuning entry points (tcpck_ex.hip in libtcpck.so) and
// their measurement twins (tcpck_ex_probe.hip in libtcpck_probe.so).  Not
// installed.
//
// The router (tcpck::api::batch_*_ex) plans each batch (tcpck_plan.h: the
// product's kernel policy and nothing else) and launches the plan; the probe
// library passes it a Hooks value to reach the measured alternatives (header
// pass forms, fused headers on explicit kernels), the product library always
// passes Hooks{}.  A batch's images travel as one Images value: the ImageSpan
// the launchers take (tcpck_internal.h) and the host-only layout hints.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

#include "tcpck.h"
#include "tcpck_internal.h"
#include "tcpck_plan.h"

struct tcpck_ctx {
  int device = 0;
  int num_cus = 256;

  // end-to-end (host batch) pipeline state, created lazily
  std::mutex mu;
  hipStream_t s[2] = {nullptr, nullptr};
  uint8_t *stage[2] = {nullptr, nullptr};     // image bytes
  uint8_t *stage_out[2] = {nullptr, nullptr}; // results
  uint64_t *stage_off[2] = {nullptr, nullptr};
  uint32_t *stage_len[2] = {nullptr, nullptr};
  uint64_t stage_bytes = 0;
  uint64_t stage_images = 0;
  uint64_t chunk_bytes = 64ull << 20;

  // FILL without a results buffer (the reference's insert stores only into the
  // packet, socket-manager.cc:9-10) where AUTO's form reads the results back
  // (the stream writes them, the write-through field pass stores them): the
  // results go to one of kScratchSlots ctx-owned slots, allocated on first use.
  // A call takes an idle slot (or, all busy, the next in turn) under
  // `scratch_mu`, then holds that slot's own mutex while it waits on the
  // slot's event, launches and records the event again -- so FILLs from
  // several threads on several streams overlap, and a slot's reuse still waits
  // for its previous user's work.  Batches of more images run in chunks.
  struct ScratchSlot {
    std::mutex mu;
    uint16_t *buf = nullptr;
    hipEvent_t ev = nullptr;
    bool used = false;  // ev recorded at least once
  };
  static constexpr int kScratchSlots = 4;
  std::mutex scratch_mu;
  ScratchSlot scratch[kScratchSlots];
  uint64_t scratch_images = 0;
  unsigned scratch_next = 0;
  // A refused allocation is not latched: the call runs the in-stream form and
  // the slots are tried again after kScratchRetry more out-less FILLs.
  uint64_t scratch_retry_at = 0;   // out-less FILL count from which allocation is tried again
  uint64_t scratch_calls = 0;      // out-less FILLs that asked for a slot
  uint64_t scratch_refusals = 0;   // allocations refused so far (tcpck_probe_scratch_state)
  int probe_scratch_fail = 0;      // probe library: refuse this many more allocation attempts (tests)

  // Pipelined FILL (round 6): the batch in K chunks, chunk i's stream pass on
  // the caller's stream and its field pass on `pipe` after the event
  // pipe_ev[i], so the field pass of chunk i runs beside the stream of chunk
  // i + 1; pipe_ev[K] joins `pipe` back into the caller's stream.  Created on
  // first use; one pipelined call is enqueued at a time (pipe_mu).
  static constexpr int kPipeMax = 32;
  std::mutex pipe_mu;
  hipStream_t pipe = nullptr;
  hipEvent_t pipe_ev[kPipeMax + 1] = {};
  int pipe_prio = 0;               // the pipe stream's priority (probe: tcpck_probe_set_fill_pipe)
  int probe_fill_pipe = -1;        // probe library: K (0/1 off, -1 AUTO's rule)
  bool probe_pipe_one_stream = false;  // probe library: the K chunks one after the other on the caller's stream

  // probe library: deliver's launch grid (tcpck_probe_set_deliver_grid; 0: the
  // launcher's rule) and the split of the last deliver launch, {blocks,
  // per_block, rem}.  The product library leaves all five at 0.
  uint64_t probe_deliver_run = 0, probe_deliver_max_blocks = 0;
  uint64_t probe_deliver_split[3] = {0, 0, 0};

  // probe library only (tcpck_ex_probe.hip): per-wave time stamp buffer, and the
  // side stream + events of the concurrent RECEIVE form
  void *dbg = nullptr;
  uint8_t *probe_side = nullptr;   // rstream 33 / 34: the field blocks' side buffer (64 B per image)
  uint64_t probe_side_cap = 0;
  std::mutex side_mu;
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};

namespace tcpck {
namespace host {
// The exact sum of the little-endian u16 words of p[0, n) (n even), host code
// (tcpck_host.cc); tcpck_checksum16 finishes it.
uint64_t word_sum(const uint8_t *p, size_t n);
}  // namespace host

namespace api {

constexpr uint64_t kScratchImages = 8ull << 20;  // 16 MiB of u16 results: C5's 8M images in one chunk
constexpr uint64_t kScratchRetry = 64;           // out-less FILLs between allocation attempts after a refusal

// (the measurement hooks, Hooks: tcpck_plan.h)
// probe library: tcpck_batch_*_ex param bit selecting Hooks::patch_reverse
constexpr int kProbeParamPatchReverse = 1 << 27;

int hip_status(hipError_t e);

inline bool valid_op_mode(int op, int mode) {
  return (op == TCPCK_OP_CHECKSUM || op == TCPCK_OP_FILL || op == TCPCK_OP_VERIFY) &&
         (mode == TCPCK_MODE_REF || mode == TCPCK_MODE_RFC1071);
}

// Saves the calling thread's current device, switches to `device`, restores.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device);
  ~DeviceGuard();
  hipError_t status() const { return ok_; }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;

 private:
  int prev_ = -1;
  hipError_t ok_ = hipSuccess;
};

// Where a batch's images are (ImageSpan, tcpck_internal.h: what the launchers
// take), with what only the host reads: the caller's layout hint or nullptr.
struct Images : ImageSpan {
  const tcpck_layout *layout;
  uint64_t total_bytes;  // these images' share of layout->total_bytes (sub)
  bool lone;             // one image cut from a gapped fixed layout (sub): the batch's plan is not its plan

  static Images fixed(uint8_t *arena, uint64_t stride, uint32_t len, uint64_t count) {
    return {{arena, nullptr, nullptr, stride, 0, count, len}, nullptr, 0, false};
  }
  static Images list(uint8_t *arena, const uint64_t *offsets, const uint32_t *lengths, uint64_t base, uint64_t count,
                     const tcpck_layout *layout) {
    return {{arena, offsets, lengths, 0, base, count, 0}, layout, layout ? layout->total_bytes : 0, false};
  }

  // Images [k0, k0 + n).  An offset list keeps the flags and the length bounds
  // of its hint, and its byte hint scales with its image count, so its typical
  // image -- the quantity AUTO chooses by -- is the whole batch's and every
  // chunk runs the same form (tcpck_tuning.h).  A lone image of a gapped fixed
  // layout has no stride to speak of: it is one packed image, to be planned
  // on its own (`lone`).
  Images sub(uint64_t k0, uint64_t n) const {
    Images im = *this;
    im.count = n;
    if (is_fixed()) {
      im.arena = arena + k0 * stride;
      if (n == 1 && stride != len) {
        im.stride = len;
        im.lone = true;
      }
    } else {
      im.offsets = offsets + k0;
      im.lengths = lengths + k0;
      im.total_bytes = static_cast<uint64_t>(static_cast<unsigned __int128>(total_bytes) * n / count);
    }
    return im;
  }
};

// The fixed-layout argument checks every entry point shares.
// (count - 1) * stride + len, the end of the last image, does not fit 64 bits:
inline bool fixed_end_overflows(uint64_t stride, uint32_t len, uint64_t count) {
  return count > 1 && stride > (UINT64_MAX - len) / (count - 1);
}
// Even `len` and `stride`, images of at least `min_len` bytes that do not
// overlap, and no overflow.  One image: its stride is never read and becomes
// `len` (the run kernels assume stride >= len).
inline bool valid_fixed(uint64_t &stride, uint32_t len, uint64_t count, uint32_t min_len) {
  if (((len | stride) & 1) || len < min_len || (count > 1 && stride < len) || fixed_end_overflows(stride, len, count))
    return false;
  if (count == 1) stride = len;
  return true;
}
// ... for the calls that touch only the first `bytes` of each slot and take no
// image length: one image's stride may be anything even.
inline bool valid_fixed_slots(uint64_t stride, uint32_t bytes, uint64_t count) {
  return count == 1 ? (stride & 1) == 0 : valid_fixed(stride, bytes, count, 0);
}

// The validated device-batch entry points (tcpck_tuning.h semantics).
int batch_fixed_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, uint64_t stride, uint32_t len, uint64_t count,
                   void *d_out, int kernel, int param, hipStream_t stream, const Hooks &hk);
int batch_var_ex(tcpck_ctx *ctx, int op, int mode, void *d_arena, const uint64_t *d_offsets,
                 const uint32_t *d_lengths, uint64_t count, void *d_out, const tcpck_layout *layout, int kernel,
                 int param, hipStream_t stream, const Hooks &hk);
int batch_receive_ex(tcpck_ctx *ctx, int mode, void *d_arena, uint64_t stride, uint32_t len,
                     const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, uint8_t *d_ok,
                     void *d_hdr, const tcpck_layout *layout, int kernel, int param, hipStream_t stream,
                     const Hooks &hk);
// batch_receive_ex's checks without the launch (TCPCK_OK or the error status)
int check_receive(const tcpck_ctx *ctx, int mode, const void *d_arena, uint64_t &stride, uint32_t len,
                  const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count, const uint8_t *d_ok,
                  const void *d_hdr);

// The routed launches behind them (device already selected, arguments valid):
// the batch's plan (plan_fixed / plan_var), then the plan's launches.
hipError_t run(tcpck_ctx *ctx, int op, int mode, const Images &im, void *out, int kernel, int param, hipStream_t s,
               uint8_t *hdr, const Hooks &hk);
// A FILL from its batch's plan (the FILL front below batch_*_ex's scratch
// decision; declared for tests/cpp/router_trace.cc).
hipError_t fill(tcpck_ctx *ctx, const Plan &plan, int mode, const Images &im, uint16_t *out, int kernel, int param,
                hipStream_t s, const Hooks &hk);

}  // namespace api
}  // namespace tcpck
