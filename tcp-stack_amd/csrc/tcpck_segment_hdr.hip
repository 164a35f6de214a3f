// tcpck_segment_hdr.hip -- zero-copy segmentation: a send ring of many
// connections -> one finished 32-B header per segment, the payload checksummed
// where it lies in the send arena (tcpck_batch_segment_headers, include/tcpck.h).
//
// Reference (filixi/TCP-stack), per data segment: the same send path
// tcpck_segment.hip restates (GetAsTcpPacket include/tcp-buffer.h:82-98, Estab's
// kSend src/state.cc:167-184, TcpHeaderH2N, the checksum of
// include/socket-manager.h:259-260) -- without the copy of the payload: the send
// stream stays put until it is acknowledged (TcpSendingBuffer::Ack,
// include/tcp-buffer.h:51-68), so a datagram leaves as a two-entry iovec, the
// header from here and the payload from the arena.
//
// The ring is `n_seg` segments, cut c owning ring indices [first_c, first_c +
// ceil(bytes_c / seg)).  There is no output image, so the kernel is a read
// stream with a trickle of writes (46 B per segment):
//   * runs of whole groups of 4 consecutive ring indices per wave
//     (dev::count_split over the groups: every run's headers start on a 128-B
//     line of the header array), blocks in XCD-chunked order;
//   * a wave finds its first cut by binary search over `first`, then walks cut
//     by cut with wave-uniform state; only sound cuts (tcpck_segment_hdr.h)
//     count, every other ring index gets zeros;
//   * the part of a cut inside the run is one contiguous byte range, covered by
//     16-B chunks aligned in the arena, one per lane and step, U steps of nt
//     buffer loads in flight; the range's first and last chunk, where they are
//     partial, are read dword by dword inside the range (the last 2 B as a
//     half dword), so nothing outside the cut is read;
//   * seg >= 16 puts at most one segment boundary inside a chunk: the lane
//     keeps the chunk's sum after it (`hi`); one 64-lane inclusive scan per
//     step, and segment i's payload sum is P(end_i) - P(end_{i-1}), P(end) =
//     carry + incl - hi of the chunk holding the end, read with one cross-lane
//     pull per ending segment, the previous end by DPP wave_shr:1; u32
//     differences are exact, so RFC 1071 mode folds them;
//   * the lane that resolves a segment adds the template's word sum (once per
//     cut, the three replaced fields zero), the length and seq words, finishes
//     the checksum and stages header, offset and length in the wave's LDS ring;
//     64 staged segments leave at once: 2 KiB of headers as 16-B stores over
//     whole lines, then the offsets, lengths and checksums.
// Cuts of one or two segments take a step each with idle lanes.
// Jumbo segments (>= 8 KiB) take segment_wide_kernel's split: W waves stream
// one segment, partial sums met in LDS, one lane emits the header.
#include <algorithm>

#include "tcpck_api_internal.h"
#include "tcpck_device.h"
#include "tcpck_internal.h"
#include "tcpck_segment_hdr.h"

namespace tcpck {

namespace {

using dev::kBlock;
using dev::kWavesPerBlock;
using dev::u32x4;

constexpr uint32_t kSlots = 128;         // staged segments per wave: < 64 wait, <= 64 resolve per round
constexpr uint32_t kNone = 0xFFFFFFF0u;  // out of every buffer range: no traffic, reads 0

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
__device__ __forceinline__ uint32_t halves(uint32_t w) { return (w & 0xFFFFu) + (w >> 16); }
__device__ __forceinline__ uint32_t uniform(uint32_t x) {
  return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)));
}

// A cut's fields as wave-uniform values.
struct Cut {
  uint64_t offset;
  uint32_t bytes, seq0, tmpl, first, nseg;
};
__device__ __forceinline__ Cut load_cut(const SegmentHdrArgs &a, uint32_t c) {
  const tcpck_send_cut &s = a.cuts[c];
  Cut r;
  r.offset = (static_cast<uint64_t>(uniform(static_cast<uint32_t>(s.offset >> 32))) << 32) |
             uniform(static_cast<uint32_t>(s.offset));
  r.bytes = uniform(s.bytes);
  r.seq0 = uniform(s.seq0);
  r.tmpl = uniform(s.tmpl);
  r.first = uniform(s.first);
  r.nseg = seghdr::segments_of(r.bytes, a.seg);
  return r;
}
__device__ __forceinline__ bool sound(const SegmentHdrArgs &a, uint32_t c) {
  return uniform(seghdr::sound(a.cuts, a.n_cuts, c, a.seg, a.payload_bytes, a.n_tmpl, a.n_seg) ? 1u : 0u) != 0;
}

// The smallest cut index in [0, n_cuts] whose `first` exceeds g (binary search:
// `first` ascends over the sound cuts).  An unsound cut's `first` says nothing,
// so a probe that lands on one reads the next sound cut within four instead.
__device__ __forceinline__ uint32_t first_cut_after(const SegmentHdrArgs &a, uint32_t g) {
  uint32_t lo = 0, hi = a.n_cuts;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t p = mid;
    for (uint32_t k = 0; k < 4 && p + 1 < a.n_cuts && !sound(a, p); ++k) ++p;
    if (!sound(a, p)) p = mid;
    if (uniform(a.cuts[p].first) <= g) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The template's eight dwords (wave-uniform) and its word sum with TcpLength,
// seq and the checksum field zero.
struct Tmpl {
  uint32_t w[8];
  uint32_t sum;
};
__device__ __forceinline__ Tmpl load_tmpl(const SegmentHdrArgs &a, uint32_t t) {
  const uint32_t *p = reinterpret_cast<const uint32_t *>(a.tmpl + 32ull * t);
  Tmpl r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = uniform(p[i]);
  r.sum = halves(r.w[0]) + halves(r.w[1]) + (r.w[2] & 0xFFFFu) + halves(r.w[3]) + halves(r.w[5]) + halves(r.w[6]) +
          (r.w[7] >> 16);
  return r;
}

// One finished segment: the header's two halves and (len << 16) | checksum.
template <int MODE>
__device__ __forceinline__ uint32_t finish_header(const Tmpl &t, uint32_t seq, uint32_t len, uint32_t payload_sum,
                                                  u32x4 &h0, u32x4 &h1) {
  const uint32_t nlen = bswap16(len), nseq = bswap32(seq);
  const uint32_t c = dev::finish<MODE>(t.sum + nlen + halves(nseq) + payload_sum);
  h0 = u32x4{t.w[0], t.w[1], (t.w[2] & 0x0000FFFFu) | (nlen << 16), t.w[3]};
  h1 = u32x4{nseq, t.w[5], t.w[6], (t.w[7] & 0xFFFF0000u) | c};
  return (len << 16) | c;
}

// The 16-B chunk at byte 16 q of the resource, of which only [lo, hi) belongs
// to the range (a partial first or last chunk): the dwords inside it, the last
// 2 B as a half dword, nothing else read.
__device__ __forceinline__ u32x4 load_edge(__amdgpu_buffer_rsrc_t r, uint32_t q, uint32_t lo, uint32_t hi) {
  uint32_t d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t b = 16 * q + 4 * k;
    d[k] = 0u;
    if (b >= lo && b + 4 <= hi) d[k] = __builtin_amdgcn_raw_buffer_load_b32(r, static_cast<int>(b), 0, 0);
    else if (b >= lo && b + 2 <= hi) d[k] = static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b16(r, static_cast<int>(b), 0, 0));
  }
  return u32x4{d[0], d[1], d[2], d[3]};
}

// A byte range of the arena as a stream of arena-aligned 16-B chunks: the
// resource starts at the aligned address at or below the range, `lead` bytes
// before it, and ends with it.
struct Range {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t lead, end, nch;  // the range is [lead, end) of the resource; chunks
  __device__ __forceinline__ bool edge(uint32_t q) const {
    return (q == 0 && lead) || (q + 1 == nch && (end & 15u));
  }
  __device__ __forceinline__ u32x4 load(uint32_t q) const {
    return dev::load16_buf_nt(rsrc, (q < nch && !edge(q)) ? q << 4 : kNone, 0);
  }
};
__device__ __forceinline__ Range make_range(const uint8_t *payload, uint64_t start, uint32_t len) {
  const uint8_t *p = payload + start;
  Range r;
  r.lead = uniform(static_cast<uint32_t>(reinterpret_cast<uint64_t>(p)) & 15u);
  r.end = r.lead + len;
  r.nch = (r.end + 15) >> 4;
  r.rsrc = dev::make_rsrc(p - r.lead, r.end);
  return r;
}

template <int U, int MODE>
__global__ void __launch_bounds__(kBlock) segment_hdr_kernel(SegmentHdrArgs a) {
  __shared__ u32x4 s_hdr[kWavesPerBlock][2 * kSlots];
  __shared__ uint64_t s_off[kWavesPerBlock][kSlots];
  __shared__ uint32_t s_lc[kWavesPerBlock][kSlots];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = uniform(threadIdx.x >> 6);
  const uint32_t bid = dev::ordered_block(blockIdx.x, gridDim.x, a.order);
  const uint64_t wid = static_cast<uint64_t>(bid) * kWavesPerBlock + wv;
  uint64_t kb, ke;
  dev::count_split(wid, a.per_wave, a.rem, kb, ke);  // groups of 4 ring indices
  const uint32_t gb = static_cast<uint32_t>(min(4 * kb, a.n_seg));
  const uint32_t ge = static_cast<uint32_t>(min(4 * ke, a.n_seg));
  if (gb >= ge) return;
  const uint32_t S = a.seg;

  // ring indices [gb, done) are staged or out, [gb, flushed) are out
  uint32_t done = gb, flushed = gb;
  auto stage = [&](uint32_t g, u32x4 h0, u32x4 h1, uint64_t off, uint32_t lc) {
    const uint32_t slot = (g - gb) & (kSlots - 1);
    s_hdr[wv][2 * slot] = h0;
    s_hdr[wv][2 * slot + 1] = h1;
    s_off[wv][slot] = off;
    s_lc[wv][slot] = lc;
  };
  // whole batches of 64, and at the run's end the rest
  auto flush = [&](bool all) {
    while (done - flushed >= 64 || (all && done > flushed)) {
      const uint32_t n = min(done - flushed, 64u);
      __builtin_amdgcn_wave_barrier();  // staged by other lanes
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t t = lane + 64 * h;  // 16-B unit of the batch
        if (t < 2 * n) {
          const uint32_t slot = (flushed - gb + (t >> 1)) & (kSlots - 1);
          *reinterpret_cast<u32x4 *>(a.hdr + 32ull * flushed + 16ull * t) = s_hdr[wv][2 * slot + (t & 1)];
        }
      }
      if (lane < n) {
        const uint32_t slot = (flushed - gb + lane) & (kSlots - 1);
        const uint64_t g = static_cast<uint64_t>(flushed) + lane;
        const uint32_t lc = s_lc[wv][slot];
        if (a.pay_off) a.pay_off[g] = s_off[wv][slot];
        if (a.pay_len) a.pay_len[g] = lc >> 16;
        if (a.out) a.out[g] = static_cast<uint16_t>(lc);
      }
      __builtin_amdgcn_wave_barrier();  // the slots are staged again
      flushed += n;
    }
  };
  auto zeros_to = [&](uint32_t g1) {  // ring indices no sound cut claims
    while (done < g1) {
      const uint32_t n = min(g1 - done, 64u);
      if (lane < n) stage(done + lane, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, 0, 0);
      done += n;
      flush(false);
    }
  };

  const uint32_t after = first_cut_after(a, gb);
  for (uint32_t c = after ? after - 1 : 0; c < a.n_cuts && done < ge; ++c) {
    if (!sound(a, c)) continue;
    const Cut cut = load_cut(a, c);
    if (cut.first >= ge) break;
    if (cut.first + cut.nseg <= done) {
      // an idle connection: many may follow, so search for the last cut that
      // starts at or before `done` and go on from there
      if (cut.nseg == 0) {
        const uint32_t nx = first_cut_after(a, done);
        if (nx >= c + 3) c = nx - 2;
      }
      continue;
    }
    if (cut.first > done) zeros_to(cut.first);
    // segments [i0, i1) of the cut are this run's: one byte range of the arena
    const uint32_t i0 = done - cut.first;
    const uint32_t nsg = min(ge, cut.first + cut.nseg) - done;
    const uint32_t at0 = i0 * S;  // < bytes
    const uint32_t rlen = min(cut.bytes - at0, nsg * S);
    const Range r = make_range(a.payload, cut.offset + at0, rlen);
    const Tmpl tm = load_tmpl(a, cut.tmpl);
    const uint32_t nsteps = (r.nch + 63) >> 6;
    const uint32_t g0 = done;

    u32x4 ring[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ring[u] = r.load((static_cast<uint32_t>(u) << 6) + lane);

    uint32_t carry = 0, p_last = 0, jn = 0;
    for (uint32_t sb = 0; sb < nsteps; sb += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t st = sb + u;
        const uint32_t q = (st << 6) + lane;
        u32x4 w = ring[u];
        if (q >= r.nch) w = u32x4{0u, 0u, 0u, 0u};
        else if (r.edge(q)) w = load_edge(r.rsrc, q, r.lead, r.end);
        // the segment boundary inside (16 q, 16 q + 16] of the range, if any: x
        // = the chunk's end relative to the range, b = the last boundary <= x
        const uint32_t x = 16 * q + 16 - r.lead;
        const uint32_t k = a.magic ? (__umulhi(x, a.magic) >> a.shift) : (x >> a.shift);
        const uint32_t b = k * S;
        const uint32_t nd = (k >= 1 && k < nsg && b + 16 > x) ? (b + 16 - x) >> 2 : 4u;  // dwords before it, 1..4
        const uint32_t t0 = dev::dot2_u16(w.x, 0u), t1 = dev::dot2_u16(w.y, t0), t2 = dev::dot2_u16(w.z, t1),
                       t3 = dev::dot2_u16(w.w, t2);
        const uint32_t hi = t3 - (nd == 4 ? t3 : (nd == 3 ? t2 : (nd == 2 ? t1 : t0)));
        const uint32_t incl = dev::wave_inclusive_scan(t3);
        const uint32_t pv = incl - hi;  // P at the chunk's boundary, less the carry
        // segments ending in this step: lane l takes segment jn + l of the range
        // (64 boundaries and the range's end can share a step: a second round)
        for (;;) {
          const uint32_t ie = jn + lane;
          const bool last = ie + 1 == nsg;
          const uint32_t end = last ? rlen : (ie + 1) * S;  // relative to the range
          const uint32_t e = (r.lead + end - 1) >> 4;        // the chunk holding its last byte
          const bool inb = ie < nsg && (e >> 6) == st;
          const uint64_t bal = __ballot(inb);
          if (!bal) break;
          const int src = static_cast<int>(e & 63u);
          const uint32_t at_b = static_cast<uint32_t>(__shfl(static_cast<int>(pv), src, 64));
          const uint32_t at_e = static_cast<uint32_t>(__shfl(static_cast<int>(incl), src, 64));
          const uint32_t pe = carry + (last ? at_e : at_b);  // the range's end: everything up to it
          const uint32_t pprev = static_cast<uint32_t>(
              __builtin_amdgcn_update_dpp(static_cast<int>(p_last), static_cast<int>(pe), 0x138, 0xF, 0xF, false));
          if (inb) {
            const uint32_t at = (i0 + ie) * S;
            u32x4 h0, h1;
            const uint32_t lc = finish_header<MODE>(tm, cut.seq0 + at, end - ie * S, pe - pprev, h0, h1);
            stage(g0 + ie, h0, h1, cut.offset + at, lc);
          }
          const uint32_t cnt = static_cast<uint32_t>(__popcll(bal));
          p_last = dev::read_lane(pe, cnt - 1);
          jn += cnt;
          done += cnt;
          flush(false);
          if (cnt < 64) break;
        }
        carry += dev::read_lane(incl, 63);
        ring[u] = r.load(((st + U) << 6) + lane);
      }
    }
  }
  zeros_to(ge);
  flush(true);
}

// Jumbo segments: the block's W waves stream ONE segment together, wave w
// taking its 1-KiB steps w, w + W, ..., the W partial sums met in LDS, thread 0
// emitting the header; the block then takes the next ring index (grid-stride).
template <int W, int U, int MODE>
__global__ void __launch_bounds__(64 * W) segment_hdr_wide_kernel(SegmentHdrArgs a) {
  __shared__ uint32_t s_part[W];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = uniform(threadIdx.x >> 6);
  const uint32_t S = a.seg;
  const uint32_t bid = dev::ordered_block(blockIdx.x, gridDim.x, a.order);
  for (uint64_t g64 = bid; g64 < a.n_seg; g64 += gridDim.x) {
    const uint32_t g = static_cast<uint32_t>(g64);
    const uint32_t after = first_cut_after(a, g);
    bool claimed = after > 0 && sound(a, after - 1);
    Cut cut{};
    if (claimed) {
      cut = load_cut(a, after - 1);
      claimed = g - cut.first < cut.nseg;  // (first <= g: the search)
    }
    u32x4 h0{0, 0, 0, 0}, h1{0, 0, 0, 0};
    uint64_t off = 0;
    uint32_t lc = 0;
    if (claimed) {  // block-uniform
      const uint32_t at = (g - cut.first) * S;  // < bytes
      const uint32_t len = min(S, cut.bytes - at);
      off = cut.offset + at;
      const Range r = make_range(a.payload, off, len);
      const uint32_t nsteps = (r.nch + 63) >> 6;
      u32x4 ring[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ring[u] = r.load(((wv + W * u) << 6) + lane);
      uint32_t acc = 0;
      for (uint32_t sb = wv; sb < nsteps; sb += W * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t st = sb + W * u;
          const uint32_t q = (st << 6) + lane;
          u32x4 w = ring[u];
          if (q >= r.nch) w = u32x4{0u, 0u, 0u, 0u};
          else if (r.edge(q)) w = load_edge(r.rsrc, q, r.lead, r.end);
          acc += dev::ref_chunk_sum_dot(w);  // < 2^32 for a segment < 64 KiB: exact
          ring[u] = r.load(((st + W * U) << 6) + lane);
        }
      }
      acc = dev::group_sum<64>(acc);
      if (lane == 0) s_part[wv] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) sum += s_part[i];
        lc = finish_header<MODE>(load_tmpl(a, cut.tmpl), cut.seq0 + at, len, sum, h0, h1);
      }
      __syncthreads();  // s_part is rewritten for the next segment
    }
    if (threadIdx.x == 0) {
      u32x4 *h = reinterpret_cast<u32x4 *>(a.hdr + 32ull * g);
      h[0] = h0;
      h[1] = h1;
      if (a.pay_off) a.pay_off[g] = off;
      if (a.pay_len) a.pay_len[g] = lc >> 16;
      if (a.out) a.out[g] = static_cast<uint16_t>(lc);
    }
  }
}

template <int W, int U, int MODE>
hipError_t launch_wide(const SegmentHdrArgs &a, uint32_t num_cus, hipStream_t stream) {
  static const uint32_t per_cu = [] {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, segment_hdr_wide_kernel<W, U, MODE>, 64 * W, 0) != hipSuccess ||
        nb < 1)
      nb = 1;
    return static_cast<uint32_t>(nb);
  }();
  // one block per segment up to 64 x the resident grid, segment_wide_kernel's rule
  const uint64_t blocks = std::min<uint64_t>(a.n_seg, static_cast<uint64_t>(per_cu) * num_cus * 64);
  hipLaunchKernelGGL((segment_hdr_wide_kernel<W, U, MODE>), dim3(static_cast<uint32_t>(blocks)), dim3(64 * W), 0, stream,
                     a);
  return hipGetLastError();
}

template <int U, int MODE>
hipError_t launch_run(SegmentHdrArgs a, hipStream_t stream) {
  // runs of about 16 KiB of payload, in whole groups of 4 ring indices (a
  // 128-B line of headers): 12 MSS segments, 1024 16-B ones.  One run per
  // wave, the dispatcher refilling freed slots; a run stays far below the 2^30
  // bytes its u32 arithmetic allows.
  const uint64_t groups = (a.n_seg + 3) / 4;
  const uint64_t run = std::max<uint64_t>(1, ((16u << 10) + 2 * a.seg) / (4 * a.seg));
  const uint64_t waves = (groups + run - 1) / run;
  const uint64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > 0xFFFFFFFFull) return hipErrorInvalidValue;
  a.per_wave = groups / (blocks * kWavesPerBlock);
  a.rem = groups % (blocks * kWavesPerBlock);
  hipLaunchKernelGGL((segment_hdr_kernel<U, MODE>), dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_segment_headers(int mode, SegmentHdrArgs a, uint32_t num_cus, hipStream_t stream) {
  if (a.n_seg == 0) return hipSuccess;
  uint32_t sh = 0;
  while ((2u << sh) <= a.seg) ++sh;  // floor(log2 seg)
  a.shift = sh;
  a.magic = (a.seg & (a.seg - 1)) == 0 ? 0u : static_cast<uint32_t>(((uint64_t{1} << (32 + sh)) + a.seg - 1) / a.seg);
  a.order = 4u;  // groups of 16 blocks per XCD
  // W waves per jumbo segment as tcpck_segment.hip measured them (16 from 16 KiB, 4 from 8 KiB)
  if (a.seg >= 16384)
    return mode == kRef ? launch_wide<16, 2, kRef>(a, num_cus, stream) : launch_wide<16, 2, kRfc1071>(a, num_cus, stream);
  if (a.seg >= 8192)
    return mode == kRef ? launch_wide<4, 4, kRef>(a, num_cus, stream) : launch_wide<4, 4, kRfc1071>(a, num_cus, stream);
  return mode == kRef ? launch_run<4, kRef>(a, stream) : launch_run<4, kRfc1071>(a, stream);
}

}  // namespace tcpck

using tcpck::api::DeviceGuard;
using tcpck::api::hip_status;

extern "C" int tcpck_batch_segment_headers(tcpck_ctx *ctx, int mode, const void *d_payload, uint64_t payload_bytes,
                                           uint32_t seg, const tcpck_send_cut *d_cuts, uint32_t n_cuts,
                                           const void *d_tmpl, uint32_t n_tmpl, uint64_t n_seg, void *d_hdr,
                                           uint64_t *d_pay_off, uint32_t *d_pay_len, uint16_t *d_out,
                                           tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  const int rc = tcpck::seghdr::check(mode, d_payload, payload_bytes, seg, d_cuts, n_cuts, d_tmpl, n_tmpl, n_seg, d_hdr,
                                      d_pay_off, d_pay_len, d_out);
  if (rc != TCPCK_OK || n_seg == 0) return rc;
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::SegmentHdrArgs a{};
  a.payload = static_cast<const uint8_t *>(d_payload);
  a.payload_bytes = payload_bytes;
  a.cuts = d_cuts;
  a.tmpl = static_cast<const uint8_t *>(d_tmpl);
  a.hdr = static_cast<uint8_t *>(d_hdr);
  a.pay_off = d_pay_off;
  a.pay_len = d_pay_len;
  a.out = d_out;
  a.n_seg = n_seg;
  a.n_cuts = n_cuts;
  a.n_tmpl = n_tmpl;
  a.seg = seg;
  return hip_status(tcpck::launch_segment_headers(mode, a, static_cast<uint32_t>(ctx->num_cus),
                                                  static_cast<hipStream_t>(stream)));
}
