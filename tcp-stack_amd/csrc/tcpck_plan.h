// tcpck_plan.h -- the batch router's policy as plain host code (no HIP,
// tcpck_plan.cc): the layout predicates of the kernels, and the plan of one
// batch -- which kernel runs with which param, and which passes go before and
// after it -- that tcpck_router.hip launches from.  Included by tcpck_internal.h.
// Not installed.
#pragma once

#include <stdint.h>

#include "tcpck.h"

namespace tcpck {

// ---- seg kernel: any layout, G lanes per image, U loads of 16 B in flight ----
enum SegShape : int {
  kShapeSmall = 0,   // G = 8,  U = 2  : images up to ~256 B
  kShapeMss = 1,     // G = 16, U = 6  : images up to ~4 KiB (Ethernet MSS)
  kShapeJumbo = 2,   // G = 64, U = 4  : 4-6 KiB images
  kShapeWave2 = 3,   // G = 64, U = 2  : tuning
  kShapeG32 = 4,     // G = 32, U = 3  : tuning
  kShapeG4 = 5,      // G = 4,  U = 8  : tuning
  kShapeW4 = 6,      // 4 waves per image, U = 4  : jumbo images
  kShapeW8 = 7,      // 8 waves per image, U = 4  : jumbo images
  kShapeW16 = 8,     // 16 waves per image, U = 2 : jumbo images
  kShapeW16U4 = 9,   // 16 waves per image, U = 4 : tuning
  kShapeW2 = 10,     // 2 waves per image, U = 4  : jumbo images
  kNumShapes = 11
};

// seg's shape for a (typical) image length
SegShape shape_for_len(uint64_t typical_len);
// gstream (tcpck_gstream.hip): fixed stride == len, len a power of two in
// [32, 1024] or a multiple of 16 B up to 240 B, 16-B aligned arena
bool gstream_applies(const uint8_t *arena, uint64_t stride, uint32_t len);
// sstream's fixed slots (tcpck_sstream.hip): stride % 16 == 0, stride >= len
bool sstream_fixed_applies(uint64_t stride, uint32_t len);
// gstream variants AUTO picks (launch_gstream, tcpck_internal.h)
constexpr int kGstreamDefaultLoads = 0x80;
constexpr int kGstreamWriteBack = 0x401;

namespace api {

// Measurement hooks (libtcpck_probe.so only; the product passes Hooks{}).
struct Hooks {
  bool fuse_any_hdr = false;     // RECEIVE, explicit kernel: fuse the headers into any kernel that can
                                 // (sstream's after-the-verdicts conversion, HDR 1)
  bool hdr_after = false;        // RECEIVE into a header array: the separate header pass after VERIFY (the
                                 // product runs it first under AUTO, tcpck_plan.cc header_form)
  bool hdr_first_explicit = false;  // ... first with an explicit VERIFY kernel too (the product runs it after
                                    // an explicit kernel, so a rejected choice leaves the header array as it was)
  uint32_t hdr_store_bits = 0;   // HeaderArgs::store_bits of the header pass
  bool patch_reverse = false;    // FILL's field pass in reverse image order (PatchArgs::reverse)
  int fill_pipe = -1;            // pipelined FILL chunks: -1 AUTO's rule, 0 / 1 off, K > 1 K chunks
  bool pipe_one_stream = false;  // ... every chunk's passes on the caller's stream (the chunking cost alone)
};

// FILL's form: the field zeroed and stored by the stream kernel; or the stream
// in its deferred form (results only), then the write-through field pass; or
// the kernel's CHECKSUM pass, then the field pass deriving each checksum from
// the old field (PatchArgs::update).
enum class Fill { kNone, kInStream, kDeferred, kUpdate };
// RECEIVE's header form: emitted by the VERIFY kernel itself (sstream), or the
// header pass before / after it.
enum class Hdr { kNone, kFused, kFirst, kAfter };

// Everything one batch's launches need, decided once.  The launch order is
// fixed: the header pass (kFirst), the stream kernel -- or, for a rejected
// request, hipErrorInvalidValue in its place --, the field pass, the header
// pass (kAfter).
struct Plan {
  int kernel = 0;           // resolved, never TCPCK_KERNEL_AUTO
  int param = 0;            // as that kernel's launcher takes it (seg: the shape resolved)
  int op = 0;               // what the stream kernel runs: CHECKSUM for FILL's update form, VERIFY for RECEIVE
  Fill fill = Fill::kNone;
  Hdr hdr = Hdr::kNone;
  bool rejected = false;    // the kernel / param does not take this request
  bool field_pass() const { return fill == Fill::kDeferred || fill == Fill::kUpdate; }
};

// The plan of a fixed-layout batch / an offset-list batch (layout: the
// caller's hint or nullptr) for the caller's kernel and param
// (tcpck_tuning.h); has_out / has_hdr: a results buffer / a header array exist.
Plan plan_fixed(int op, int mode, const uint8_t *arena, uint64_t stride, uint32_t len, uint64_t count, bool has_out,
                bool has_hdr, int kernel, int param, const Hooks &hk);
Plan plan_var(int op, int mode, const tcpck_layout *layout, uint64_t count, bool has_out, bool has_hdr, int kernel,
              int param, const Hooks &hk);

}  // namespace api

}  // namespace tcpck
