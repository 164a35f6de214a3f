// tcpck_deliver.hip -- the receive path's consumer, batched: the payloads of
// the accepted images of a receive batch copied into the connection's receive
// stream (tcpck_batch_deliver, include/tcpck.h).
//
// Reference (filixi/TCP-stack), per accepted packet:
//   SocketInternal::Accept()                include/socket-internal.h:323-334
//     TcpLength > 0: recv_buffer_.insert(end, packet->begin(), packet->end()),
//     a byte-by-byte append to a std::deque<char>
// Which images are accepted, and where in the stream each payload goes, is the
// state machine's serial chain (src/state.cc:195-223): the host planner
// (tcpck_deliver_plan.cc) writes dst[k]; this kernel is the per-byte copy.
//
// Image k's payload is bytes [32, len_k) of the image, 2-B aligned and any
// value mod 16; so is its destination dst[k].  Lanes map to the 16-B ALIGNED
// DESTINATION chunks of an image's range [d, d + P): an interior chunk is one
// whole aligned 16-B store, the head and tail chunks are stored in 8/4/2-B
// pieces inside the range, so no byte outside a delivered range is written.
// The chunk's source bytes start at a 2-B aligned address: when (source -
// destination) % 4 == 0 one dword-aligned 16-B buffer load brings them; when it
// is 2, the 16 B and the dword after them are loaded from 2 B below and every
// output dword is a funnel shift (v_alignbit) of two neighbours.
//
// One run of whole images per BLOCK, walked in groups of 64 images:
//   * lane l of every wave reads image l's descriptor (offset, length, dst) and
//     counts its chunks (0: SKIP, odd dst, range past recv_bytes, no payload);
//     a 64-lane scan lays the group's chunks end to end;
//   * the group's steps of 64 chunks go round the block's W waves (wave w takes
//     steps w, w + W, ...: a jumbo image is streamed by the whole block, 64-B
//     payloads share a step), U steps of loads in flight per wave;
//   * a lane finds its chunk's image by a 6-probe search of the scan held in
//     the lanes (ds_bpermute) and pulls that image's fields the same way.
// Source and destination go through raw buffer resources whose range is the
// group's own extent -- [lowest image start, highest image end) of the arena,
// [lowest, highest delivered byte) of the receive stream -- so the hardware's
// range check backs the index arithmetic; a group whose images lie further
// apart than 2^30 B (unsorted lists over a > 1 GiB arena) is walked in several
// passes, each over the images near the first one pending.  A tail chunk whose
// 16-B load would pass the group's extent is read dword by dword, each dword
// holding a byte of the image.  The next group's descriptors are loaded while
// the current group streams.
#include <algorithm>

#include "tcpck_api_internal.h"
#include "tcpck_device.h"
#include "tcpck_internal.h"

namespace tcpck {

namespace {

using dev::u32x4;

constexpr int kDeliverWaves = 4;
constexpr uint32_t kNone = 0xFFFFFFF0u;  // out of every buffer range: no traffic, reads 0
constexpr uint32_t kHalfWindow = 1u << 29;

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = min(x, static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), m, 64)));
  return x;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = max(x, static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), m, 64)));
  return x;
}
__device__ __forceinline__ uint32_t pull(uint32_t x, uint32_t from) {
  return static_cast<uint32_t>(__shfl(static_cast<int>(x), static_cast<int>(from), 64));
}

// One ring slot: the chunk's five source dwords (from 2 B below the chunk when
// the source sits 2 mod 4 against the destination), its destination offset and
// what to store of it.
struct Slot {
  u32x4 v;
  uint32_t v4;
  uint32_t x;     // destination offset of the chunk, relative to the pass's base
  uint32_t meta;  // bits 0-7 word mask (0: no chunk), bits 8-12 funnel shift in bits (0 / 16)
};

template <int W, int U>
__global__ void __launch_bounds__(64 * W) deliver_kernel(DeliverArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
  const uint32_t bid = dev::ordered_block(blockIdx.x, gridDim.x, a.order);
  uint64_t kb, ke;
  dev::count_split(bid, a.per_block, a.rem, kb, ke);
  if (kb >= ke) return;
  const uint64_t arena = reinterpret_cast<uint64_t>(static_cast<const uint8_t *>(a.im.arena));

  // image kb + lane's descriptor; invalid ones come back with ln = 0
  auto descriptor = [&](uint64_t k, uint64_t &off, uint32_t &ln, uint64_t &d) {
    off = 0, ln = 0, d = TCPCK_DELIVER_SKIP;
    if (k < ke) {
      d = a.dst[k];
      if (d != TCPCK_DELIVER_SKIP) {
        off = a.im.start(k);
        ln = a.im.length(k);
      }
    }
  };

  uint64_t n_off, n_d;
  uint32_t n_ln;
  descriptor(kb + lane, n_off, n_ln, n_d);
  for (uint64_t g0 = kb; g0 < ke; g0 += 64) {
    const uint64_t off = n_off, d = n_d;
    const uint32_t ln = n_ln;
    descriptor(g0 + 64 + lane, n_off, n_ln, n_d);  // the next group's, in flight over this one
    // the payload and whether it is delivered at all: the whole range inside
    // [0, recv_bytes), even everywhere (odd values would split a u16 word)
    const uint32_t P = ln > 32 ? ln - 32 : 0;
    // (a length past 16 MiB is no TCP image: skipped, which keeps the u32 arithmetic below exact)
    bool pending = P > 0 && ln <= (1u << 24) && !((ln | off | d) & 1) && P <= a.recv_bytes && d <= a.recv_bytes - P;
    const uint64_t src = arena + off;  // the image's first byte

    for (uint64_t bal = __ballot(pending); bal; bal = __ballot(pending)) {
      // this pass: the pending images within 2^29 B of the first one, on both sides
      const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(bal));
      const uint64_t s0 = dev::read_lane64(src, leader) - kHalfWindow;  // (differences only: may wrap)
      const uint64_t d0 = dev::read_lane64(d, leader) - kHalfWindow;
      const bool cand = pending && src - s0 < 2ull * kHalfWindow && d - d0 < 2ull * kHalfWindow;
      const uint64_t sbase = (s0 + wave_min_u32(cand ? static_cast<uint32_t>(src - s0) : ~0u)) & ~uint64_t{3};
      const uint64_t dbase = (d0 + wave_min_u32(cand ? static_cast<uint32_t>(d - d0) : ~0u)) & ~uint64_t{15};
      const uint32_t img_rel = static_cast<uint32_t>(src - sbase);  // < 2^30 + 4 for candidates
      const uint32_t d_rel = static_cast<uint32_t>(d - dbase);      // < 2^30 + 16
      const uint32_t e_rel = d_rel + P;
      // the arena extent the pass may read (whole dwords: sbase is 4-B aligned,
      // a dword holding an image byte lies in that byte's page) and the receive
      // stream extent it may write (exactly up to the last delivered byte)
      const uint32_t srec = (wave_max_u32(cand ? img_rel + ln : 0u) + 3u) & ~3u;
      const uint32_t drec = wave_max_u32(cand ? e_rel : 0u);
      const auto rin = dev::make_rsrc(reinterpret_cast<const void *>(sbase), srec);
      const auto rout = dev::make_rsrc(a.recv + dbase, drec);
      // source offset of destination offset x of the image: delta + x
      const uint32_t delta = img_rel + 32u - d_rel;
      const uint32_t nch = cand ? ((e_rel + 15u) >> 4) - (d_rel >> 4) : 0u;
      const uint32_t incl = dev::wave_inclusive_scan(nch);  // <= 64 x 2^20 chunks (+ 64: a range may straddle one more)
      const uint32_t excl = incl - nch;
      const uint32_t T = dev::read_lane(incl, 63);
      const uint32_t nsteps = (T + 63) >> 6;

      auto load_step = [&](uint32_t t) -> Slot {
        Slot s;
        s.v = u32x4{0u, 0u, 0u, 0u};
        s.v4 = 0;
        s.x = 0;
        s.meta = 0;
        if (t >= nsteps) return s;  // wave-uniform
        const uint32_t q = (t << 6) + lane;
        const bool live = q < T;
        // the chunk's image: the first lane whose inclusive count passes q
        uint32_t i = 0;
#pragma unroll
        for (uint32_t step = 32; step >= 1; step >>= 1)
          if (pull(incl, i + step - 1) <= q) i += step;
        // (i <= 63; a lane with q >= T has no chunk and stays idle)
        const uint32_t i_excl = pull(excl, i), i_d = pull(d_rel, i), i_e = pull(e_rel, i), i_delta = pull(delta, i);
        const uint32_t x = ((i_d >> 4) + (q - i_excl)) << 4;
        const uint32_t lo = max(x, i_d), hi = min(x + 16u, i_e);
        const uint32_t sh = i_delta & 2u;
        const uint32_t at = i_delta + x - sh;  // 4-B aligned, >= 16 B into the image
        const uint32_t reach = at + (sh ? 20u : 16u);
        // a tail chunk whose whole load would pass the extent: dword by dword
        const bool slow = live && reach > srec;
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rin, static_cast<int>(live && !slow ? at : kNone), 0, 2);
        s.v = u32x4{v.x, v.y, v.z, v.w};
        s.v4 = __builtin_amdgcn_raw_buffer_load_b32(rin, static_cast<int>(live && !slow && sh ? at + 16u : kNone), 0, 2);
        if (slow) {
          // dword j holds destination bytes [x - sh + 4 j, + 4): read it when one of them is wanted
          uint32_t r[5];
#pragma unroll
          for (uint32_t j = 0; j < 5; ++j)
            r[j] = x + 4u * j < hi + sh ? __builtin_amdgcn_raw_buffer_load_b32(rin, static_cast<int>(at + 4u * j), 0, 0)
                                        : 0u;
          s.v = u32x4{r[0], r[1], r[2], r[3]};
          s.v4 = r[4];
        }
        s.x = x;
        s.meta = live ? (dev::word_mask(static_cast<int32_t>(lo - x), static_cast<int32_t>(hi - x)) | (sh << 11)) : 0u;
        return s;
      };

      Slot ring[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ring[u] = load_step(wv + W * static_cast<uint32_t>(u));
      for (uint32_t g = wv; g < nsteps; g += W * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t t = g + W * static_cast<uint32_t>(u);
          const Slot s = ring[u];
          const uint32_t wm = s.meta & 0xFFu, bits = (s.meta >> 8) & 31u;
          // bits 0: the chunk as loaded; 16: every dword from the upper half of
          // its own and the lower half of the next
          const uint32_t o0 = __builtin_amdgcn_alignbit(s.v.y, s.v.x, bits);
          const uint32_t o1 = __builtin_amdgcn_alignbit(s.v.z, s.v.y, bits);
          const uint32_t o2 = __builtin_amdgcn_alignbit(s.v.w, s.v.z, bits);
          const uint32_t o3 = __builtin_amdgcn_alignbit(s.v4, s.v.w, bits);
          typedef unsigned v4u __attribute__((ext_vector_type(4)));
          typedef unsigned v2u __attribute__((ext_vector_type(2)));
          if (wm == 0xFFu) {
            const v4u o = {o0, o1, o2, o3};
            __builtin_amdgcn_raw_buffer_store_b128(o, rout, static_cast<int>(s.x), 0, 0);
          } else if (wm) {  // head or tail chunk (or both): pieces inside the range
            const uint32_t o[4] = {o0, o1, o2, o3};
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
              const uint32_t m = (wm >> (4 * h)) & 15u;
              if (m == 15u) {
                const v2u p = {o[2 * h], o[2 * h + 1]};
                __builtin_amdgcn_raw_buffer_store_b64(p, rout, static_cast<int>(s.x + 8u * h), 0, 0);
                continue;
              }
#pragma unroll
              for (uint32_t j = 2 * h; j < 2 * h + 2; ++j) {
                const uint32_t mj = (wm >> (2 * j)) & 3u;
                if (mj == 3u)
                  __builtin_amdgcn_raw_buffer_store_b32(o[j], rout, static_cast<int>(s.x + 4u * j), 0, 0);
                else if (mj == 1u)
                  __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(o[j]), rout, static_cast<int>(s.x + 4u * j),
                                                        0, 0);
                else if (mj == 2u)
                  __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(o[j] >> 16), rout,
                                                        static_cast<int>(s.x + 4u * j + 2u), 0, 0);
              }
            }
          }
          ring[u] = load_step(t + W * U);
        }
      }
      pending = pending && !cand;
    }
  }
}

}  // namespace

hipError_t launch_deliver(DeliverArgs a, uint32_t num_cus, uint64_t run_forced, uint64_t max_blocks_forced,
                          uint64_t *split, hipStream_t stream) {
  if (a.im.count == 0) return hipSuccess;
  constexpr int W = kDeliverWaves, U = 4;
  static const uint32_t per_cu = [] {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, deliver_kernel<W, U>, 64 * W, 0) != hipSuccess || nb < 1)
      nb = 1;
    return static_cast<uint32_t>(nb);
  }();
  // runs of up to one group (64 images) per block while that fills the device
  // four times over; a large batch gets 64 x the resident grid and longer runs
  const uint64_t resident = static_cast<uint64_t>(per_cu) * num_cus;
  // (tests force either through the probe library to reach the group walk at small counts)
  const uint64_t run =
      run_forced ? run_forced : std::min<uint64_t>(64, std::max<uint64_t>(1, a.im.count / (resident * 4)));
  const uint64_t cap = max_blocks_forced ? max_blocks_forced : resident * 64;
  const uint64_t blocks = std::min<uint64_t>(a.im.count / run + (a.im.count % run != 0), cap);
  a.per_block = a.im.count / blocks;
  a.rem = a.im.count % blocks;
  if (split) split[0] = blocks, split[1] = a.per_block, split[2] = a.rem;
  a.order = 4u;  // groups of 16 blocks per XCD
  hipLaunchKernelGGL((deliver_kernel<W, U>), dim3(static_cast<uint32_t>(blocks)), dim3(64 * W), 0, stream, a);
  return hipGetLastError();
}

}  // namespace tcpck

using tcpck::api::DeviceGuard;
using tcpck::api::hip_status;

extern "C" int tcpck_batch_deliver(tcpck_ctx *ctx, const void *d_arena, uint64_t stride, uint32_t len,
                                   const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count,
                                   const uint64_t *d_dst, void *d_recv, uint64_t recv_bytes, tcpck_stream stream) {
  if (!ctx) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!d_arena || !d_dst || !d_recv) return TCPCK_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d_arena) & 1) || (reinterpret_cast<uintptr_t>(d_recv) & 15)) return TCPCK_EINVAL;
  if (d_offsets) {
    if (!d_lengths) return TCPCK_EINVAL;
  } else {
    if (d_lengths || (stride & 1) || (len & 1) || len < TCPCK_HEADER_BYTES || stride < len) return TCPCK_EINVAL;
    if (count > UINT64_MAX / stride) return TCPCK_EINVAL;
  }
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  tcpck::DeliverArgs a{};
  // (the span's arena is shared with the launchers that write; this kernel only reads through it)
  a.im = {static_cast<uint8_t *>(const_cast<void *>(d_arena)), d_offsets, d_lengths, stride, 0, count, len};
  a.dst = d_dst;
  a.recv = static_cast<uint8_t *>(d_recv);
  a.recv_bytes = recv_bytes;
#ifdef TCPCK_PROBE  // the probe library: the grid a test set, and the split it reads back
  return hip_status(tcpck::launch_deliver(a, static_cast<uint32_t>(ctx->num_cus), ctx->probe_deliver_run,
                                          ctx->probe_deliver_max_blocks, ctx->probe_deliver_split,
                                          static_cast<hipStream_t>(stream)));
#else
  return hip_status(tcpck::launch_deliver(a, static_cast<uint32_t>(ctx->num_cus), 0, 0, nullptr,
                                          static_cast<hipStream_t>(stream)));
#endif
}
