// tcpck_host_batch.hip -- the end-to-end calls on host memory
// (tcpck_host_batch_*, include/tcpck.h): the batch in chunks through the
// context's two staging buffers, H2D -> the routed kernels (tcpck_router.hip)
// -> D2H on two streams, and the same over several contexts, one per GPU.
// These calls use ctx-owned streams and staging and are serialised per ctx.
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

using tcpck::api::DeviceGuard;
using tcpck::api::Hooks;
using tcpck::api::Images;
using tcpck::api::hip_status;
using tcpck::api::valid_op_mode;

namespace {

size_t out_elem(int op) { return op == TCPCK_OP_VERIFY ? 1 : 2; }

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

// Patches bytes 28-29 of host images after a FILL computed on the device
// (the device filled its staging copy; the host image is the caller's).
void patch_fields(const Images &host, const uint16_t *res) {
  for (uint64_t k = 0; k < host.count; ++k) {
    const uint64_t o = host.offsets ? host.offsets[k] : k * host.stride;
    const uint32_t l = host.lengths ? host.lengths[k] : host.len;
    if (l >= 30) std::memcpy(host.arena + o + 28, &res[k], 2);
  }
}

// Where a host batch's results go: the caller's buffer, or -- a FILL without
// one -- `fill_res`, which the host field patch reads.
uint8_t *results_buffer(int op, void *h_out, uint64_t count, std::vector<uint16_t> &fill_res) {
  if (op == TCPCK_OP_FILL && !h_out) fill_res.resize(count);
  return h_out ? static_cast<uint8_t *>(h_out) : reinterpret_cast<uint8_t *>(fill_res.data());
}

// The end of a host batch whose chunks were enqueued with status `e`: waits
// for both streams (also after an error), then patches a FILL's fields into
// the caller's images `host`.
int finish_batch(tcpck_ctx *ctx, hipError_t e, int op, const Images &host, const uint8_t *out_bytes) {
  for (int i = 0; i < 2; ++i) {
    hipError_t e2 = hipStreamSynchronize(ctx->s[i]);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return hip_status(e);
  if (op == TCPCK_OP_FILL) patch_fields(host, reinterpret_cast<const uint16_t *>(out_bytes));
  return TCPCK_OK;
}

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

// ---- batched, host memory: chunked H2D -> kernel -> D2H on two streams ---------
int tcpck_host_batch_fixed(tcpck_ctx *ctx, int op, int mode, void *h_arena, uint64_t stride,
                           uint32_t len, uint64_t count, void *h_out) {
  if (!ctx || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || (!h_out && op != TCPCK_OP_FILL)) return TCPCK_EINVAL;
  if (!tcpck::api::valid_fixed(stride, len, count, op == TCPCK_OP_FILL ? 30 : 0)) return TCPCK_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard g(ctx->device);
  if (g.status() != hipSuccess) return hip_status(g.status());
  const uint64_t step = std::max<uint64_t>(stride, 2);
  const uint64_t per = std::max<uint64_t>(1, ctx->chunk_bytes / step);
  const uint64_t chunk_imgs = std::min(per, count);
  int rc = ensure_stage(ctx, (chunk_imgs - 1) * stride + len, chunk_imgs);
  if (rc) return rc;
  std::vector<uint16_t> fill_res;
  auto *arena = static_cast<uint8_t *>(h_arena);
  uint8_t *out_bytes = results_buffer(op, h_out, count, fill_res);
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
    e = tcpck::api::run(ctx, op, mode, Images::fixed(ctx->stage[slot], stride, len, n), ctx->stage_out[slot],
                        TCPCK_KERNEL_AUTO, 0, s, nullptr, Hooks{});
    if (e != hipSuccess) break;
    e = hipMemcpyAsync(out_bytes + k0 * es, ctx->stage_out[slot], n * es, hipMemcpyDeviceToHost, s);
  }
  return finish_batch(ctx, e, op, Images::fixed(arena, stride, len, count), out_bytes);
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
  auto *arena = static_cast<uint8_t *>(h_arena);
  uint8_t *out_bytes = results_buffer(op, h_out, count, fill_res);
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
    e = tcpck::api::run(ctx, op, mode,
                        Images::list(ctx->stage[slot], ctx->stage_off[slot], ctx->stage_len[slot], lo, n, &lay),
                        ctx->stage_out[slot], TCPCK_KERNEL_AUTO, 0, s, nullptr, Hooks{});
    if (e != hipSuccess) break;
    e = hipMemcpyAsync(out_bytes + k0 * es, ctx->stage_out[slot], n * es, hipMemcpyDeviceToHost, s);
    k0 = k1;
  }
  return finish_batch(ctx, e, op, Images::list(arena, h_offsets, h_lengths, 0, count, nullptr), out_bytes);
}

// ---- host batches over several contexts (one per GPU) ---------------------------

int tcpck_host_batch_fixed_multi(tcpck_ctx *const *ctxs, int n_ctx, int op, int mode, void *h_arena,
                                 uint64_t stride, uint32_t len, uint64_t count, void *h_out) {
  if (!valid_ctx_list(ctxs, n_ctx) || !valid_op_mode(op, mode)) return TCPCK_EINVAL;
  if (count == 0) return TCPCK_OK;
  if (!h_arena || (!h_out && op != TCPCK_OP_FILL)) return TCPCK_EINVAL;
  // (the rest of the fixed-layout checks: each shard's tcpck_host_batch_fixed)
  if (tcpck::api::fixed_end_overflows(stride, len, count)) return TCPCK_EINVAL;
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

}  // extern "C"
