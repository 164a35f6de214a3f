// tcpck_plan.cc -- the batch router's policy (tcpck_plan.h): plain host C++,
// no HIP call and no context state, so it can be driven without a GPU
// (tests/cpp/router_trace.cc).
#include "tcpck_plan.h"

#include "tcpck_tuning.h"

namespace tcpck {

// Images above 4 KiB: W waves per image, one block round (W x 4 KiB) just
// covering the image (scripts/xcd_probe.py --what jumbo,
// profiles/r01/jumbo_probe.log: 6 KiB W2 90.6%, 12 KiB W4 91.2%, 32 KiB W8
// 90.9%, 64 KiB W16 91.1%, against 80-85% for one wave per image).
SegShape shape_for_len(uint64_t typical_len) {
  if (typical_len <= 256) return kShapeSmall;
  if (typical_len <= 4096) return kShapeMss;
  if (typical_len <= 8192) return kShapeW2;
  if (typical_len <= 16384) return kShapeW4;
  if (typical_len <= 32768) return kShapeW8;
  return kShapeW16;
}

bool gstream_applies(const uint8_t *arena, uint64_t stride, uint32_t len) {
  const bool pow2 = (len & (len - 1)) == 0;
  return stride == len && len >= 32 && len <= 1024 && (len & 15u) == 0 && (pow2 || len <= 240) &&
         (reinterpret_cast<uintptr_t>(arena) & 15u) == 0;
}

bool sstream_fixed_applies(uint64_t stride, uint32_t len) {
  return stride >= len && len >= 2 && (stride & 15u) == 0 && stride <= (1u << 24);
}

namespace api {
namespace {

// ---- kernel selection (AUTO; measurements in profiles/DESIGN_history_r01-r04.md section 4) ------------
// reference mode:
//   fixed, stride == len   < 512 B vvstream (prefix table), 512 B..4 KiB
//                          rstream (scalar boundary walk), larger seg with
//                          W waves per image (~4 KiB per wave) where the
//                          image fills seg's steps, else rstream
//   fixed, stride > len    small gaps vvstream (gaps streamed as virtual
//                          images), larger gaps sstream (compacted slot
//                          stream) in slots of a multiple of 16 B, else seg
//                          with 8 lanes per image
//   packed variable        vvstream, every op
//   sorted variable        (TCPCK_LAYOUT_SORTED: receive slots) sstream for
//                          CHECKSUM / VERIFY
// everything else -- unordered offsets, gaps in variable layouts, RFC 1071
// mode, variable or gapped layouts of images above 16 KiB (where one wave per
// image already streams whole 1 KiB steps) -- seg.
constexpr uint64_t kRunMaxLen = 32768;       // packed variable layouts, typical image: above, seg
constexpr uint64_t kFixedRunMaxLen = 4096;   // packed fixed: rstream up to here; above, seg with W waves
                                             // per image where the image fills its steps (jumbo_on_seg;
                                             // C4 64 KiB: W16 91% vs rstream 85-88%, 6 KiB: W2 90.6% vs
                                             // 87.0%, profiles/r01/jumbo_probe.log), else rstream
// Policy parameters.  Every kernel takes its runs in the XCD-chunked block
// order (dev::ordered_block, groups of 16 blocks per XCD): each XCD streams
// compact regions instead of every eighth run (C2 86.3% -> 90.6%, C3 82.7 ->
// 84.1%, C4 85.5 -> 87.4%, profiles/r01/xcd_*.log; the HBM bytes do not
// change, PMC).  rstream also reads each run's first line with the default
// cache policy: that line is the previous run's last line, and the
// neighbour's last step then finds it in L2 (PMC bytes x1.015 -> x1.000;
// C2 90.9 -> 93.1% warm with the whole first step; since round 5 only the
// first line, 92.3% cold and warm), and large batches keep runs of 4-8 KiB with up to
// 1024 x the resident grid (C5: 256x, 84.7% at 32x -> 92.5%,
// profiles/r01/oversub_c5_first_step.log, split_probe.log); vvstream the
// same with runs >= 8 KiB (C3 86.3 -> 89.5%, profiles/r01/xcd_first_step_probe.log).
constexpr int kRstreamPolicy = 20;       // v_dot2 sums, buffer loads, XCD-chunked order, L2-kept first line
constexpr int kRstreamDeferFill = 25;    // FILL: kRstreamPolicy's stream to out, then the 2-B write-through field pass
constexpr int kVvPolicy = 4 | 8 | 16;    // size policy, XCD-chunked order, L2-kept first line
constexpr int kSegXcdOrder = 1 << 24;    // seg: XCD-chunked order
// seg W16 on packed jumbo images (C4): image k's chunk walk starts at 1-KiB
// step (29 k) mod 64 and wraps (SegArgs::rot), so the blocks in flight --
// consecutive images, 64 KiB apart -- read different offsets at the same time:
// C4 90.4 -> 92.7 % (multipliers = 1 mod 16 gain nothing, the other odd ones
// 91.8-92.9 %; W8 at 32 KiB loses 1-1.5 points, so W16 only;
// scripts/c4_rot_sweep.py, profiles/r03/c4_rot_sweep*.log)
constexpr int kSegW16Rot = 29;
// FILL of small images: nearly every line holds a checksum field, so the
// run kernels read every step with the default cache policy; the line is then
// still in L2 when the field store lands and leaves as a whole line instead of
// a masked partial write (scripts/keep_probe.py, profiles/r01/keep_probe.log:
// 96 B 20.4 -> 29.9 % of the roof, 192 B 28.6 -> 38.1 %, 320 B 38.0 -> 44.1 %,
// 480 B +0.6 %, the C3 mix -3.7 %: bytes per image up to 448)
constexpr uint64_t kFillKeepMaxLen = 448;
constexpr int kVvKeep = 32;              // vvstream: kFill reads with the default policy
constexpr int kVvDeferFill = 64;         // vvstream: kFill writes the results only, the field pass follows
// FILL with a results buffer on the run kernels: the stream writes only the
// results and the write-through field pass stores the fields, for (typical)
// images of at least this many bytes; smaller images pay more for 1M-per-
// 38-us scattered field stores than the in-stream stores cost them
constexpr uint64_t kDeferFillMinLen = 512;
// packed fixed images: vvstream's deferred form from 320 B up to 1 KiB, where
// it beats the in-stream forms and rstream's (round-4 re-check after the
// write-through field pass, scripts/fill_policy_sweep.py,
// profiles/r04/fill_policy_sweep.log, us per 1.5 GB: 320 B 448 -> 430, 384 B
// 427 -> 397, 448 B 408 -> 366, 512 B 347 (gstream) -> 328, 640 B 359
// (rstream 25) -> 322, 768 B 318 -> 308; 1 KiB stays on rstream 25: 279 vs 284)
constexpr uint64_t kVvDeferPackedMin = 320, kVvDeferPackedEnd = 1024;
constexpr int kSstreamDeferFill = 128;   // sstream: kFill writes the results only, the field pass follows
// variable layouts: vvstream's in-stream zeroing costs ~25 us per 1M images, so
// its deferred form pays only for larger images (C3's mean 732 B: 718 -> 702
// us; 256-1024 B: 700 -> 740 us; 1492 B: 365 -> 262 us; profiles/r03/fill_forms.log)
constexpr uint64_t kDeferFillMinVar = 1024;
constexpr int kSstreamHdrStream = 32;    // sstream RECEIVE: headers from the stream's registers
constexpr uint64_t kHdrStreamMaxLen = 256;  // ... for (typical) images up to this length

// Packed fixed images above 4 KiB: seg's W-wave shapes stream W KiB of an
// image per step (shape_for_len: W = 2, 4, 8, 16 up to 8, 16, 32, 64 KiB), so
// an image that ends early in its last step wastes the rest of that step --
// 9000 B on W4 reads as 3 x 4 KiB: 72 % of the roof against rstream's 90 %
// (profiles/r01/jumbo_fit_probe.log).  seg keeps the sizes it fills to >= 85 %
// (W16: only in four steps);
// FILL only from 24 KiB (below, rstream's batched field stores win even at a
// perfect fit: 8-24 KiB 77-81 % vs 82-84 %).
static bool jumbo_on_seg(int op, uint64_t len) {
  if (len > 65536) return true;
  const uint64_t step = len <= 8192 ? 2048 : (len <= 16384 ? 4096 : (len <= 32768 ? 8192 : 16384));
  const uint64_t steps = (len + step - 1) / step;
  const bool fits = 100 * len >= 85 * steps * step && (step < 16384 || steps == 4);  // W16: 48 KiB 81 vs 83 %
  return op == TCPCK_OP_FILL ? fits && len > 24576 : fits;
}

// AUTO's kernel for a fixed layout: sets kernel (from TCPCK_KERNEL_AUTO) and
// its param (measurements in profiles/DESIGN_history_r01-r04.md section 4).
void pick_fixed(int op, int mode, const uint8_t *arena, uint64_t stride, uint32_t len, int &kernel, int &param) {
  if (mode == TCPCK_MODE_RFC1071 && stride == len && len >= 512 && len <= kFixedRunMaxLen) {
    // RFC 1071 on packed fixed images: rstream's prefix is an exact u32 word
    // sum, so its image differences fold like any sum (C2 in RFC 1071 mode at
    // the REF rate instead of seg's; profiles/r02/rfc_probe.log)
    kernel = TCPCK_KERNEL_RSTREAM;
    param = kRstreamPolicy;
  } else if (mode == TCPCK_MODE_RFC1071 && stride == len && len >= 2 && len < 512 &&
             (op != TCPCK_OP_FILL || len >= 30)) {
    // RFC 1071 on small packed images: vvstream's fixed mode with exact u32 prefix tables
    kernel = TCPCK_KERNEL_VVSTREAM;
    param = kVvPolicy;
  }
  if (kernel == TCPCK_KERNEL_AUTO) {
    // jumbo images in slots with small gaps (9000 B in 9216-B slots): vvstream
    // streams the gaps as virtual images, 86 % against seg's 70 % (FILL 78 vs
    // 64 %; profiles/r01/jumbo_layout_probe.log, jumbo_layout_fill_probe.log)
    const bool jumbo_hull = stride > len && len <= 65536 && 16 * stride <= 17 * static_cast<uint64_t>(len);
    // jumbo images in slots with larger gaps: the compacted slot stream where
    // the slot is a multiple of 16 B (9000 B in 16-KiB slots 74.2 -> 85.0 %,
    // FILL 65.6 -> 79.0 %, profiles/r02/slot_probe_ss3.log), else seg
    const bool jumbo_slots = stride > len && !jumbo_hull && tcpck::sstream_fixed_applies(stride, len) &&
                             (op != TCPCK_OP_FILL || len >= 30);
    // RFC 1071: slots with larger gaps (beyond vvstream's hull rule) on sstream
    // with exact u32 prefix tables; every other layout not routed above on seg
    const bool rfc_slots = mode == TCPCK_MODE_RFC1071 && stride > len && len < (1u << 17) &&
                           tcpck::sstream_fixed_applies(stride, len) && (op != TCPCK_OP_FILL || len >= 30);
    if (rfc_slots) {
      kernel = TCPCK_KERNEL_SSTREAM;
      param = 0;
    } else if (mode != TCPCK_MODE_REF || len < 2 ||
        (len > kFixedRunMaxLen && !jumbo_slots && (stride > len ? !jumbo_hull : jumbo_on_seg(op, len))) ||
        stride > (1u << 24)) {
      kernel = TCPCK_KERNEL_SEG;
      param = kSegXcdOrder;  // shape by length
      if (mode == TCPCK_MODE_REF && stride == len && len <= 65536 && op != TCPCK_OP_FILL &&
          tcpck::shape_for_len(len) == tcpck::kShapeW16)
        param |= kSegW16Rot << 8;
    } else if (stride > len) {
      // gapped fixed strides (e.g. MSS slots) (scripts/gap_probe.py,
      // profiles/r01/gap_probe.log): streaming the gaps with the images
      // (vvstream, virtual gap images) wins while they are small -- 128/96 B
      // 57% of the roof for image bytes vs seg's 39% -- else seg with 8 lanes
      // per image (1536/1492 B 81% vs 77% for the length-based shape)
      const uint64_t l = len;
      const bool hull = len < 512 ? stride <= 2 * l : (len < 1024 ? 4 * stride <= 5 * l : 16 * stride <= 17 * l);
      // (jumbo images reach here in slots: jumbo_hull -> vvstream, jumbo_slots -> sstream)
      if (hull && (op != TCPCK_OP_FILL || len >= 30)) {
        kernel = TCPCK_KERNEL_VVSTREAM;
        param = kVvPolicy | (op == TCPCK_OP_FILL && stride <= kFillKeepMaxLen ? kVvKeep : 0);
      } else if (tcpck::sstream_fixed_applies(stride, len) && (op != TCPCK_OP_FILL || len >= 30)) {
        // larger gaps in slots of a multiple of 16 B: the compacted slot stream
        // reads only the images' chunks (scripts/slot_probe.py,
        // profiles/r02/slot_probe_ss3.log, % of the roof in image bytes, seg ->
        // sstream): 1492 B in 2048-B slots 77.4 -> 83.1 % (FILL 57.7 -> 60.1),
        // in 4-KiB slots 65.7 -> 81.2 %, 96 in 256 B 39.9 -> 55.7 %
        kernel = TCPCK_KERNEL_SSTREAM;
        param = 0;
      } else {
        kernel = TCPCK_KERNEL_SEG;
        param = (tcpck::kShapeSmall + 1) | kSegXcdOrder;
      }
    } else if (op == TCPCK_OP_FILL && len <= 256 && tcpck::gstream_applies(arena, stride, len)) {
      // send-path FILL of power-of-two images, 32 B (pure ACKs) .. 256 B, and
      // of the other multiples of 16 B up to 240 B (512 B and 1 KiB: the
      // deferred-field forms since round 3's write-through field pass,
      // vvstream 328 vs 347 us and rstream 279 vs 299 us per 1.5 GB,
      // profiles/r04/fill_policy_sweep.log):
      // gstream; up to 256 B every line holds a checksum field, and reading
      // the lines with the default cache policy keeps them in L2 until the
      // field store lands, so they leave as whole lines rather than masked
      // partial writes (scripts/gstream_probe.py, profiles/r01/gstream_fill.log:
      // 32 B 21.4 -> 32 % of the roof, 256 B 33 -> 43 %, 512 B 46 -> 57 %).
      // Up to 128 B, writing every chunk back whole (twice the bytes, all of
      // them full-line writes) beats even that (profiles/r01/gstream_writeback.log:
      // 32 B 33.9 -> 41.3 %, 64 B 32.5 -> 40.2 %, 128 B 36.3 -> 40.3 %; 256 B
      // 44.7 vs 39.9 % keeps the default-policy loads).  The other multiples of
      // 16 B up to 240 B take the same rule (profiles/r01/gstream_np.log: 48 B
      // 29.0 -> 36.1 %, 96 B 29.7 -> 37.0 %; 144-240 B default-policy loads
      // 1-2 points ahead of vvstream FIXED)
      kernel = TCPCK_KERNEL_GSTREAM;
      param = len <= 128 ? tcpck::kGstreamWriteBack : (len <= 256 ? tcpck::kGstreamDefaultLoads : 0);
    } else if (len < 512 || (op == TCPCK_OP_FILL && len < kVvDeferPackedEnd)) {
      // (FILL up to 1 KiB stays here: from kVvDeferPackedMin on in vvstream's deferred form, plan_fixed)
      // packed, by image length (scripts/policy_sweep.py, profiles/r01/policy_small.log):
      // below 512 B boundaries are dense enough that resolving all of a step's
      // ends in parallel from the prefix table wins (vvstream FIXED, 80-81% at
      // 96-256 B, profiles/r01/fill_probe.log); from 512 B the scalar boundary
      // walk (rstream: 92-93% of the HBM roof on C2)
      kernel = (op == TCPCK_OP_FILL && len < 30) ? TCPCK_KERNEL_SEG : TCPCK_KERNEL_VVSTREAM;
      param = kernel == TCPCK_KERNEL_SEG ? kSegXcdOrder
                                         : kVvPolicy | (op == TCPCK_OP_FILL && len <= kFillKeepMaxLen ? kVvKeep : 0);
    } else {
      kernel = TCPCK_KERNEL_RSTREAM;
      param = kRstreamPolicy;
    }
  }
}

// AUTO's kernel for an offset list of `typical` bytes per image: sets kernel
// (from TCPCK_KERNEL_AUTO) and its param; RECEIVE into a header array on a
// ring of small datagrams: the headers from sstream's registers
// (kSstreamHdrStream, header_form below).
void pick_var(int op, int mode, const tcpck_layout *layout, uint64_t typical, bool hdr, bool two_pass, int &kernel,
              int &param) {
  const bool packed = mode == TCPCK_MODE_REF && layout && (layout->flags & TCPCK_LAYOUT_PACKED);
  // packed, reference mode: vvstream for every op (any image lengths; C3 89.1%
  // at 32x oversubscription, profiles/r01/c3_bench_r01_final.log).  The
  // packed flag must be true when set (tcpck.h); a wave whose lengths do not
  // add up to its span falls back to per-image sums, but that check cannot see
  // a gap that an overlap elsewhere in the run cancels
  if (kernel == TCPCK_KERNEL_AUTO) {
    // packed jumbo batches stay on vvstream up to a typical image of 32 KiB
    // (20000 B 86 % vs seg 76 %, FILL 82 vs 71 %; a 9000/20000/40000 mix 83
    // vs 72 %, FILL 79 vs 66 %), seg above (a 40000/60032 mix: 83.5 vs 82 %,
    // FILL 83 vs 79 %; profiles/r01/jumbo_layout_probe.log, jumbo_layout_fill_probe.log)
    const bool rfc_packed = mode == TCPCK_MODE_RFC1071 && layout && (layout->flags & TCPCK_LAYOUT_PACKED) &&
                            typical <= kRunMaxLen && layout->max_len != 0 && layout->max_len < (1u << 17) &&
                            (op != TCPCK_OP_FILL || (layout->min_len != 0 && layout->min_len >= 30));
    if (rfc_packed) {
      // RFC 1071 on packed variable layouts: vvstream with exact u32 prefix
      // tables (C3 in RFC 1071 mode, profiles/r02/rfc_probe.log)
      kernel = TCPCK_KERNEL_VVSTREAM;
      param = kVvPolicy;
    } else if (!packed && typical <= kRunMaxLen && op != TCPCK_OP_FILL && layout &&
               (layout->flags & TCPCK_LAYOUT_SORTED) &&
               (mode == TCPCK_MODE_REF || (layout->max_len != 0 && layout->max_len < (1u << 17)))) {
      // (RFC 1071 too, with exact u32 prefix tables, when every image is below 128 KiB)
      // images in order with gaps (receive slots): the compacted slot stream
      // (profiles/r02/slot_probe_ss3.log, seg -> sstream, CHECKSUM): a
      // 96/608/1492 mix in 2048-B slots 60.5 -> 70.3 %, in 1536-B slots 57.4
      // -> 68.5 %, 1492 B in 2048-B slots 73.5 -> 78.3 %; FILL stays on seg
      // (41-58 % either way: the scattered field writes bound it)
      kernel = TCPCK_KERNEL_SSTREAM;
      param = 0;
      if (op == TCPCK_OP_RECEIVE && hdr && typical <= kHdrStreamMaxLen && !two_pass) param = kSstreamHdrStream;
    } else if (!packed || typical > kRunMaxLen ||
               (op == TCPCK_OP_FILL && layout->min_len != 0 && layout->min_len < 30)) {
      kernel = TCPCK_KERNEL_SEG;
      param = kSegXcdOrder;
    } else {
      kernel = TCPCK_KERNEL_VVSTREAM;
      param = kVvPolicy | (op == TCPCK_OP_FILL && typical <= kFillKeepMaxLen ? kVvKeep : 0);
    }
  }
}

// FILL as CHECKSUM + field update (reference mode, a results buffer): the
// layout's CHECKSUM kernel at its full streaming rate, then the field pass
// derives each zero-field checksum from the old field, c = ~(~C - f) mod 2^16,
// and writes it through into the field and out[k].  Round 3 (the pass's stores
// written through, scripts/fill_defer_vv_probe.py, profiles/r03/fill_forms.log,
// % of the roof, in-stream -> update): packed variable batches on vvstream,
// whose in-stream field zeroing costs ~25 us per 1M images, gain most -- C3 53.7 ->
// 62.2 %, a 608/1492 mix 46.6 -> 69.2 %, 256-1024 B 48.3 -> 55.4 % -- so AUTO
// takes it there for typical images >= 448 B (below, vvstream's default-policy
// in-stream FILL); gapped fixed jumbo images keep it (9000 B in 9216-B slots
// 85.2 %); elsewhere the deferred-field form (the stream zeroes the fields and
// writes only the results, then the same pass stores them) ties with it or
// wins (C2 254 vs 258 us), and TCPCK_PARAM_FILL_UPDATE selects it.
constexpr uint64_t kFillUpdateMinVar = kFillKeepMaxLen;

// RECEIVE's header form.  For small images in slots sstream emits each
// host-order header from the stream's registers (one launch, the header
// bytes read once; on rings of small images, 4M 32-254-B datagrams in 256-B
// slots: 190 us against 259 with the header pass, 235 with the run's headers
// re-read after its verdicts); elsewhere a separate header pass, which
// measured faster than any fused form for MSS-sized images (header stores
// inside the read stream cost more than a separate pass: profiles/DESIGN_history_r01-r04.md "Receive
// path", profiles/r03/receive_fused_probe.log)
// (TCPCK_PARAM_RECEIVE_TWO_PASS keeps the separate pass, AUTO included).
// With an explicit kernel the product carries only the stream-register form
// (+ kSstreamHdrStream); the probe library can fuse the headers into any
// kernel that can (Hooks::fuse_any_hdr: sstream's after-the-verdicts
// conversion, HDR 1).
// Into a header array the separate pass runs FIRST: its one 128-B line
// per image (128 MB for 1M datagrams) is then still in the 256-MB Infinity
// Cache when the VERIFY stream reads the images, where after VERIFY it read
// every line from HBM again.  On a receive ring taken in turn with others (no
// step sees the previous step's lines) 158.1 -> 152.5 us per 1M datagrams of
// 96/608/1492 B in 2048-B slots (scripts/receive_ring_probe.py,
// profiles/r05/receive_ring_probe.log); the verdicts and headers are the same
// either way (the header array is not the arena).
// First under AUTO (whose choices are always valid), or with an explicit
// kernel in the probe library; with an explicit kernel the product runs it
// after VERIFY, so that a rejected kernel / param leaves the caller's header
// array untouched.  In place (no header array) it always follows VERIFY.
Hdr header_form(const Plan &p, bool has_hdr, bool is_auto, bool two_pass, const Hooks &hk) {
  if (has_hdr && p.kernel == TCPCK_KERNEL_SSTREAM && !two_pass &&
      ((hk.fuse_any_hdr && !is_auto) || (p.param & kSstreamHdrStream)))
    return Hdr::kFused;
  return has_hdr && !hk.hdr_after && (is_auto || hk.hdr_first_explicit) ? Hdr::kFirst : Hdr::kAfter;
}

Plan reject(Plan p) {
  p.rejected = true;
  return p;
}

// What every plan ends with: a stream launched in its deferred form
// (`defer`: the kernel's deferred-FILL bit in the param) is followed by the
// field pass, unless the batch's form already fixes what follows the stream
// (the update pass, the header pass first); the header pass does not follow a
// field pass (a deferred-FILL param on a RECEIVE, which the launcher rejects).
Plan finish(Plan p, bool defer) {
  if (defer && p.fill != Fill::kUpdate && p.hdr != Hdr::kFirst) p.fill = Fill::kDeferred;
  if (p.field_pass() && p.hdr == Hdr::kAfter) p.hdr = Hdr::kNone;
  return p;
}

}  // namespace

Plan plan_fixed(int op, int mode, const uint8_t *arena, uint64_t stride, uint32_t len, uint64_t count, bool has_out,
                bool has_hdr, int kernel, int param, const Hooks &hk) {
  const bool is_auto = kernel == TCPCK_KERNEL_AUTO;
  // the caller's TCPCK_PARAM_* bits, read before AUTO's choice rewrites param
  const bool two_pass = (param & TCPCK_PARAM_RECEIVE_TWO_PASS) != 0;  // RECEIVE: keep the separate header pass
  const bool instream = (param & TCPCK_PARAM_FILL_INSTREAM) != 0;     // FILL under AUTO: no field pass
  Plan p;
  p.kernel = kernel;
  p.param = param;
  p.op = op;
  if (op == TCPCK_OP_FILL) p.fill = Fill::kInStream;
  // (the update form under AUTO: gapped fixed jumbo images, see above)
  if (op == TCPCK_OP_FILL && mode == TCPCK_MODE_REF && has_out && stride >= 30 &&
      ((param & TCPCK_PARAM_FILL_UPDATE) || (is_auto && !instream && stride > len && len > 4096))) {
    p.fill = Fill::kUpdate;
    p.op = TCPCK_OP_CHECKSUM;
    p.param &= ~(TCPCK_PARAM_FILL_UPDATE | TCPCK_PARAM_FILL_INSTREAM);
  }
  if (is_auto) pick_fixed(p.op, mode, arena, stride, len, p.kernel, p.param);
  if (op == TCPCK_OP_RECEIVE) {
    p.op = TCPCK_OP_VERIFY;
    if (is_auto && has_hdr && p.kernel == TCPCK_KERNEL_SSTREAM && len <= kHdrStreamMaxLen && !two_pass)
      p.param |= kSstreamHdrStream;
    p.hdr = header_form(p, has_hdr, is_auto, two_pass, hk);
  }
  // FILL on rstream with a results buffer: the stream writes only the results,
  // then a second pass stores each field with a write-through 2-B store.
  // Scattered field stores inside a read stream, or left dirty in the
  // Infinity Cache for the next stream to write back, cost ~70 us per 1M
  // images; written through to HBM in their own pass they cost 38 us (C2:
  // 280 -> 248 us, scripts/fill_drain_probe.py, profiles/r03/fill_*.log)
  // (TCPCK_PARAM_FILL_INSTREAM keeps the in-stream form)
  const bool may_defer = is_auto && !instream && p.op == TCPCK_OP_FILL && has_out;
  switch (p.kernel) {
    case TCPCK_KERNEL_RSTREAM: {
      if (may_defer && stride >= 30 && (p.param & 0xFF) == kRstreamPolicy) p.param = (p.param & ~0xFF) | kRstreamDeferFill;
      if (stride != len || len < 16 || len > (1u << 24)) return reject(p);
      if ((p.param & 0xFF) != kRstreamDeferFill) return finish(p, false);
      // FILL: the policy's stream, the fields in a second pass
      if (p.op != TCPCK_OP_FILL || !has_out || stride < 30) return reject(p);
      p.param = (p.param & ~0xFF) | kRstreamPolicy;
      return finish(p, true);
    }
    case TCPCK_KERNEL_GSTREAM:  // stride == len, a power of two in [32, 1024], 16-B aligned arena
      if (mode != TCPCK_MODE_REF || !tcpck::gstream_applies(arena, stride, len)) return reject(p);
      return finish(p, false);
    case TCPCK_KERNEL_SSTREAM: {  // fixed slots: stride % 16 == 0, stride >= len
      if (may_defer && len >= kDeferFillMinLen) p.param |= kSstreamDeferFill;
      if (count == 1) stride = (static_cast<uint64_t>(len) + 15) & ~uint64_t{15};  // one image: never read
      if (!tcpck::sstream_fixed_applies(stride, len) || (p.op == TCPCK_OP_FILL && len < 30) ||
          (mode != TCPCK_MODE_REF && len >= (1u << 17)))
        return reject(p);
      return finish(p, (p.param & kSstreamDeferFill) != 0);
    }
    case TCPCK_KERNEL_VVSTREAM: {  // any even length: the prefix table takes any number of ends per step
      if (len == 0 || stride > (1u << 24) || (p.op == TCPCK_OP_FILL && len < 30)) return reject(p);
      if (may_defer && len >= (stride == len ? kVvDeferPackedMin : kDeferFillMinLen))
        p.param = (p.param & ~kVvKeep) | kVvDeferFill;  // (the default-policy reads served the in-stream stores)
      if (mode != TCPCK_MODE_REF && (len >= (1u << 17) || (p.param & kVvKeep))) return reject(p);
      return finish(p, (p.param & kVvDeferFill) != 0);
    }
    case TCPCK_KERNEL_SEG:
      if ((p.param & 0xFF) == 0) p.param |= tcpck::shape_for_len(len) + 1;
      return finish(p, false);
    default: return reject(p);
  }
}

Plan plan_var(int op, int mode, const tcpck_layout *layout, uint64_t count, bool has_out, bool has_hdr, int kernel,
              int param, const Hooks &hk) {
  const bool is_auto = kernel == TCPCK_KERNEL_AUTO;
  const bool two_pass = (param & TCPCK_PARAM_RECEIVE_TWO_PASS) != 0;
  const bool instream = (param & TCPCK_PARAM_FILL_INSTREAM) != 0;
  const bool hinted = layout && layout->total_bytes;
  const uint64_t typical = hinted ? layout->total_bytes / count : 1500;
  Plan p;
  p.kernel = kernel;
  p.param = param;
  p.op = op;
  if (op == TCPCK_OP_FILL) p.fill = Fill::kInStream;
  if (op == TCPCK_OP_FILL && mode == TCPCK_MODE_REF && has_out &&
      ((param & TCPCK_PARAM_FILL_UPDATE) ||
       (is_auto && !instream && hinted && (layout->flags & TCPCK_LAYOUT_PACKED) && typical >= kFillUpdateMinVar &&
        typical <= kRunMaxLen))) {
    p.fill = Fill::kUpdate;
    p.op = TCPCK_OP_CHECKSUM;
    p.param &= ~(TCPCK_PARAM_FILL_UPDATE | TCPCK_PARAM_FILL_INSTREAM);
  }
  if (is_auto) pick_var(p.op, mode, layout, typical, has_hdr, two_pass, p.kernel, p.param);
  if (op == TCPCK_OP_RECEIVE) {
    p.op = TCPCK_OP_VERIFY;
    p.hdr = header_form(p, has_hdr, is_auto, two_pass, hk);
  }
  // an offset list's stream takes its deferred form only where the field pass follows it
  const bool field_pass_follows = p.fill != Fill::kUpdate && p.hdr != Hdr::kFirst;
  switch (p.kernel) {
    case TCPCK_KERNEL_VVSTREAM: {
      if (mode != TCPCK_MODE_REF && (p.param & kVvKeep)) return reject(p);
      // (REF packed batches of typical >= 448 B take the update form above)
      if (is_auto && !instream && p.op == TCPCK_OP_FILL && has_out && typical >= kDeferFillMinVar)
        p.param |= kVvDeferFill;
      if ((p.param & kVvDeferFill) && !field_pass_follows) return reject(p);
      return finish(p, (p.param & kVvDeferFill) != 0);
    }
    case TCPCK_KERNEL_RVSTREAM:  // packed offset lists, REF, CHECKSUM / VERIFY
      if (mode != TCPCK_MODE_REF || p.op == TCPCK_OP_FILL || !has_out) return reject(p);
      return finish(p, false);
    case TCPCK_KERNEL_SSTREAM:  // any offset list (runs of <= 128 images)
      if ((p.param & kSstreamDeferFill) && !field_pass_follows) return reject(p);
      return finish(p, (p.param & kSstreamDeferFill) != 0);
    case TCPCK_KERNEL_SEG:
      if ((p.param & 0xFF) == 0) p.param |= tcpck::shape_for_len(typical) + 1;
      return finish(p, false);
    default: return reject(p);
  }
}

}  // namespace api
}  // namespace tcpck
