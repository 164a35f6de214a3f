// resend_host_test.cc -- the batched resend pass's host code under
// AddressSanitizer + UBSan: tcpck_resend_images (plain host code) and the
// argument checks of tcpck_batch_resend / tcpck_resend_scratch_bytes.  Linked
// against tcp-stack_amd/libtcpck_asan.so (tcp-stack_amd/Makefile `asan`; the
// device code is not sanitized); tests/test_resend_asan.py runs it.
//
//   resend_host_test cpu <manifest>   no device: tcpck_resend_images on the queues
//       of the manifest (expected bytes from tests/resend_np.py), every array a
//       heap block of exactly its size; every TCPCK_EINVAL path
//   resend_host_test gpu              device 0: one small tcpck_batch_resend,
//       checked against tcpck_resend_images
//
// Manifest: per queue a line `queue n n_conns has_conn fixed stride len
// arena_bytes cap mode rule total`, the arena as hex, n lines `offset length
// conn`, n_conns lines `snd_una rcv_nxt flags`, the arena after the pass as hex,
// n keep digits, and min(total, cap) lines `offset length conn src`.
// Prints "ok <n checks>" and exits 0, or names the first failed check.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "tcpck.h"

namespace {

long g_checks = 0;

#define CHECK(cond)                                                           \
  do {                                                                        \
    ++g_checks;                                                               \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)
#define CHECK_RC(expr, want)                                                                         \
  do {                                                                                               \
    ++g_checks;                                                                                      \
    const int rc_ = (expr);                                                                          \
    if (rc_ != (want)) {                                                                             \
      std::fprintf(stderr, "FAILED %s:%d: %s = %d (%s), want %d\n", __FILE__, __LINE__, #expr, rc_, \
                   tcpck_strerror(rc_), (want));                                                     \
      std::exit(1);                                                                                  \
    }                                                                                                \
  } while (0)

int hexval(int c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

// `bytes` bytes as hex, after white space ("-" stands for none)
void read_hex(FILE *f, uint8_t *out, uint64_t bytes) {
  int c = std::fgetc(f);
  while (c == ' ' || c == '\n') c = std::fgetc(f);
  if (bytes == 0) {
    CHECK(c == '-');
    return;
  }
  for (uint64_t i = 0; i < bytes; ++i) {
    const int lo = std::fgetc(f);
    CHECK(c != EOF && lo != EOF);
    out[i] = static_cast<uint8_t>(hexval(c) << 4 | hexval(lo));
    c = i + 1 < bytes ? std::fgetc(f) : 0;
  }
}

// a heap block of exactly `bytes` bytes, 16-B aligned (NULL for 0 bytes: nothing may be touched then)
template <typename T>
T *block(size_t bytes) {
  if (bytes == 0) return nullptr;
  void *p = nullptr;
  CHECK(posix_memalign(&p, 16, bytes) == 0);
  std::memset(p, 0x5A, bytes);
  return static_cast<T *>(p);
}

void queues_on_manifest(const char *path) {
  FILE *f = std::fopen(path, "r");
  CHECK(f != nullptr);
  char word[16];
  int queues = 0;
  while (std::fscanf(f, "%15s", word) == 1) {
    CHECK(std::strcmp(word, "queue") == 0);
    uint64_t v[11];
    for (auto &x : v) CHECK(std::fscanf(f, "%" SCNu64, &x) == 1);
    const uint64_t n = v[0], n_conns = v[1], has_conn = v[2], fixed = v[3], stride = v[4], len = v[5], arena_bytes = v[6],
                   cap = v[7], mode = v[8], rule = v[9], total = v[10];
    uint8_t *arena = block<uint8_t>(arena_bytes);
    read_hex(f, arena, arena_bytes);
    uint64_t *offsets = fixed ? nullptr : block<uint64_t>(8 * n);
    uint32_t *lengths = fixed ? nullptr : block<uint32_t>(4 * n), *conn = has_conn ? block<uint32_t>(4 * n) : nullptr;
    for (uint64_t k = 0; k < n; ++k) {
      uint64_t o, l, c;
      CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &o, &l, &c) == 3);
      if (offsets) offsets[k] = o, lengths[k] = static_cast<uint32_t>(l);
      if (conn) conn[k] = static_cast<uint32_t>(c);
    }
    tcpck_snd_state *snd = block<tcpck_snd_state>(16 * n_conns);
    for (uint64_t c = 0; c < n_conns; ++c) {
      uint64_t a, b, fl;
      CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &fl) == 3);
      snd[c] = tcpck_snd_state{static_cast<uint32_t>(a), static_cast<uint32_t>(b), static_cast<uint32_t>(fl), 0};
    }
    std::vector<uint8_t> want_arena(arena_bytes), want_keep(n);
    read_hex(f, want_arena.data(), arena_bytes);
    for (uint64_t k = 0; k < n; ++k) {
      int c = std::fgetc(f);
      while (c == ' ' || c == '\n') c = std::fgetc(f);
      want_keep[k] = static_cast<uint8_t>(c - '0');
    }
    const uint64_t written = std::min(total, cap);
    std::vector<uint64_t> want_off(written);
    std::vector<uint32_t> want_len(written), want_conn(written), want_src(written);
    for (uint64_t j = 0; j < written; ++j) {
      uint64_t o, l, c, s;
      CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &o, &l, &c, &s) == 4);
      want_off[j] = o, want_len[j] = static_cast<uint32_t>(l), want_conn[j] = static_cast<uint32_t>(c);
      want_src[j] = static_cast<uint32_t>(s);
    }
    // the outputs hold exactly what may be written: one byte more would be a sanitizer report
    uint8_t *keep = block<uint8_t>(n);
    uint64_t *out_off = block<uint64_t>(8 * written);
    uint32_t *out_len = block<uint32_t>(4 * written), *out_conn = block<uint32_t>(4 * written),
             *src = block<uint32_t>(4 * written);
    uint8_t dummy[16] __attribute__((aligned(16))) = {};
    uint8_t *base = arena ? arena : dummy;
    uint64_t got = 99;
    CHECK_RC(tcpck_resend_images(static_cast<int>(mode), static_cast<int>(rule), base, arena_bytes, stride,
                                 static_cast<uint32_t>(len), offsets, lengths, conn, snd, static_cast<uint32_t>(n_conns), n,
                                 keep, out_off, out_len, out_conn, src, cap, &got),
             TCPCK_OK);
    CHECK(got == total);
    CHECK(arena_bytes == 0 || std::memcmp(arena, want_arena.data(), arena_bytes) == 0);
    CHECK(n == 0 || std::memcmp(keep, want_keep.data(), n) == 0);
    CHECK(written == 0 || std::memcmp(out_off, want_off.data(), 8 * written) == 0);
    CHECK(written == 0 || std::memcmp(out_len, want_len.data(), 4 * written) == 0);
    CHECK(written == 0 || std::memcmp(out_conn, want_conn.data(), 4 * written) == 0);
    CHECK(written == 0 || std::memcmp(src, want_src.data(), 4 * written) == 0);
    // the second pass, without any output array: the same count, no byte changed
    CHECK_RC(tcpck_resend_images(static_cast<int>(mode), static_cast<int>(rule), base, arena_bytes, stride,
                                 static_cast<uint32_t>(len), offsets, lengths, conn, snd, static_cast<uint32_t>(n_conns), n,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, cap, &got),
             TCPCK_OK);
    CHECK(got == total && (arena_bytes == 0 || std::memcmp(arena, want_arena.data(), arena_bytes) == 0));
    std::free(arena), std::free(offsets), std::free(lengths), std::free(conn), std::free(snd), std::free(keep);
    std::free(out_off), std::free(out_len), std::free(out_conn), std::free(src);
    ++queues;
  }
  std::fclose(f);
  CHECK(queues >= 6);
}

void host_errors() {
  const uint64_t n = 40, stride = 64, bytes_total = n * stride;
  uint8_t *arena = block<uint8_t>(bytes_total + 2), *keep = block<uint8_t>(n + 1);
  uint64_t *offsets = block<uint64_t>(8 * n + 8), *out_off = block<uint64_t>(8 * n + 8), *total = block<uint64_t>(16);
  uint32_t *lengths = block<uint32_t>(4 * n + 4), *conn = block<uint32_t>(4 * n + 4), *out_len = block<uint32_t>(4 * n + 4),
           *out_conn = block<uint32_t>(4 * n + 4), *src = block<uint32_t>(4 * n + 4);
  tcpck_snd_state *snd = block<tcpck_snd_state>(16 * 4);
  for (uint64_t k = 0; k <= n; ++k) offsets[k] = k * stride, lengths[k] = 32, conn[k] = k % 3;
  for (int c = 0; c < 4; ++c) snd[c] = tcpck_snd_state{0, 7, 0, 0};  // 0x5A5A5A5A > 0: every image is owed
  const auto untouched = [&] {
    for (uint64_t i = 0; i < bytes_total + 2; ++i) CHECK(arena[i] == 0x5A);
    for (uint64_t i = 0; i <= n; ++i)
      CHECK(keep[i] == 0x5A && out_off[i] == 0x5A5A5A5A5A5A5A5Aull && out_len[i] == 0x5A5A5A5Au &&
            out_conn[i] == 0x5A5A5A5Au && src[i] == 0x5A5A5A5Au);
    CHECK(total[0] == 0x5A5A5A5A5A5A5A5Aull && total[1] == total[0]);
  };
  struct Args {
    int mode, rule;
    uint8_t *arena;
    uint64_t stride;
    uint32_t len;
    const uint64_t *offsets;
    const uint32_t *lengths, *conn;
    const tcpck_snd_state *snd;
    uint64_t count;
    uint64_t *out_off;
    uint32_t *out_len, *out_conn, *src;
    uint64_t *total;
  };
  const Args good{0, 0, arena, 0, 0, offsets, lengths, conn, snd, n, out_off, out_len, out_conn, src, total};
  const auto refused = [&](auto change) {
    Args a = good;
    change(a);
    CHECK_RC(tcpck_resend_images(a.mode, a.rule, a.arena, bytes_total, a.stride, a.len, a.offsets, a.lengths, a.conn, a.snd,
                                 3, a.count, keep, a.out_off, a.out_len, a.out_conn, a.src, n, a.total),
             TCPCK_EINVAL);
  };
  const auto fixed = [](Args &a, uint64_t stride, uint32_t len) { a.offsets = nullptr, a.lengths = nullptr, a.stride = stride, a.len = len; };
  const auto at = [](auto *p, size_t by) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + by); };
  refused([](Args &a) { a.mode = 2; });
  refused([](Args &a) { a.mode = -1; });
  refused([](Args &a) { a.rule = 2; });
  refused([](Args &a) { a.rule = -1; });
  refused([](Args &a) { a.count = (1ull << 31) + 1; });
  refused([](Args &a) { a.arena = nullptr; });
  refused([](Args &a) { a.snd = nullptr; });
  refused([](Args &a) { a.total = nullptr; });
  refused([](Args &a) { a.lengths = nullptr; });
  refused([](Args &a) { a.offsets = nullptr; });
  refused([&](Args &a) { fixed(a, 63, 32); });
  refused([&](Args &a) { fixed(a, 64, 33); });
  refused([&](Args &a) { fixed(a, 64, 30); });
  refused([&](Args &a) { fixed(a, 32, 34); });
  refused([&](Args &a) { fixed(a, 0, 0); });
  refused([](Args &a) { a.arena += 1; });
  refused([&](Args &a) { a.offsets = at(a.offsets, 4); });
  refused([&](Args &a) { a.lengths = at(a.lengths, 2); });
  refused([&](Args &a) { a.conn = at(a.conn, 1); });
  refused([&](Args &a) { a.snd = at(a.snd, 8); });
  refused([&](Args &a) { a.out_off = at(a.out_off, 4); });
  refused([&](Args &a) { a.out_len = at(a.out_len, 2); });
  refused([&](Args &a) { a.out_conn = at(a.out_conn, 1); });
  refused([&](Args &a) { a.src = at(a.src, 3); });
  refused([&](Args &a) { a.total = at(a.total, 4); });
  untouched();
  // nothing to do: only the count is written
  CHECK_RC(tcpck_resend_images(1, 1, nullptr, 0, 0, 0, offsets, lengths, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr,
                               nullptr, nullptr, 0, total + 1),
           TCPCK_OK);
  CHECK(total[1] == 0);
  total[1] = total[0];
  CHECK_RC(tcpck_resend_images(1, 1, nullptr, 0, 64, 32, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr,
                               nullptr, nullptr, nullptr, 0, nullptr),
           TCPCK_OK);
  untouched();
  // the alignments that are enough; the last image (offset n * 64) does not fit and is dropped untouched
  CHECK_RC(tcpck_resend_images(0, 0, arena + 2, bytes_total - 2, 0, 0, offsets + 1, lengths + 1, conn + 1, snd + 1, 3, n,
                               keep + 1, out_off + 1, out_len + 1, out_conn + 1, src + 1, n - 1, total + 1),
           TCPCK_OK);
  CHECK(total[1] == n - 1 && keep[0] == 0x5A && keep[n] == 0 && src[0] == 0x5A5A5A5Au && src[n - 1] == n - 2);
  CHECK(arena[0] == 0x5A && arena[2 + 64 + 20] == 0 && arena[2 + 64 + 23] == 7 && arena[bytes_total + 1] == 0x5A);
  uint64_t bytes_out = 5;
  CHECK_RC(tcpck_resend_scratch_bytes((1ull << 31) + 1, &bytes_out), TCPCK_EINVAL);
  CHECK_RC(tcpck_resend_scratch_bytes(8, nullptr), TCPCK_EINVAL);
  CHECK(bytes_out == 5);
  size_t small = 0, large = 0;
  CHECK_RC(tcpck_resend_scratch_bytes(0, &small), TCPCK_OK);
  CHECK_RC(tcpck_resend_scratch_bytes(1ull << 31, &large), TCPCK_OK);
  CHECK(small >= 16 && small % 16 == 0 && large % 16 == 0 && large > (1ull << 31));
  std::free(arena), std::free(keep), std::free(offsets), std::free(out_off), std::free(total), std::free(lengths);
  std::free(conn), std::free(out_len), std::free(out_conn), std::free(src), std::free(snd);
}

void gpu_checks() {
  tcpck_ctx *ctx = nullptr;
  CHECK_RC(tcpck_ctx_create(0, &ctx), TCPCK_OK);
  const uint64_t n = 3000, guard = 16, stride = 96, arena_bytes = n * stride;
  const uint32_t n_conns = 5, len = 64;
  std::mt19937_64 rng(11);
  std::vector<uint8_t> arena(arena_bytes);
  std::vector<uint32_t> conn(n);
  std::vector<tcpck_snd_state> snd(n_conns);
  for (auto &b : arena) b = static_cast<uint8_t>(rng());
  for (auto &s : snd) s = tcpck_snd_state{0x80000000u, static_cast<uint32_t>(rng()), 0, 0};
  snd[4].flags = TCPCK_SND_CLOSED;
  for (uint64_t k = 0; k < n; ++k) {
    conn[k] = rng() % 10 == 0 ? TCPCK_CONN_NONE : static_cast<uint32_t>(rng() % (n_conns + 1));
    CHECK_RC(tcpck_fill16(arena.data() + k * stride, len, 0, nullptr), TCPCK_OK);  // (seq random: about half are owed)
  }
  std::vector<uint8_t> want_arena = arena, want_keep(n);
  std::vector<uint64_t> want_off(n);
  std::vector<uint32_t> want_len(n), want_conn(n), want_src(n);
  uint64_t total = 0;
  CHECK_RC(tcpck_resend_images(0, 0, want_arena.data(), arena_bytes, stride, len, nullptr, nullptr, conn.data(), snd.data(),
                               n_conns, n, want_keep.data(), want_off.data(), want_len.data(), want_conn.data(),
                               want_src.data(), n, &total),
           TCPCK_OK);
  CHECK(total > n / 8 && total < n);
  size_t scratch_bytes = 0;
  CHECK_RC(tcpck_resend_scratch_bytes(n, &scratch_bytes), TCPCK_OK);
  void *d_arena, *d_conn, *d_snd, *d_keep, *d_off, *d_len, *d_oc, *d_src, *d_count, *d_scratch;
  CHECK_RC(tcpck_device_alloc(ctx, arena_bytes, &d_arena), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * n, &d_conn), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 16 * n_conns, &d_snd), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, n + guard, &d_keep), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 8 * (n + guard), &d_off), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * (n + guard), &d_len), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * (n + guard), &d_oc), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * (n + guard), &d_src), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 16, &d_count), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, scratch_bytes, &d_scratch), TCPCK_OK);
  std::vector<uint8_t> keep(n + guard, 0xA5);
  std::vector<uint64_t> off(n + guard, 0xA5A5A5A5A5A5A5A5ull);
  std::vector<uint32_t> ln(n + guard, 0xA5A5A5A5u), oc(n + guard, 0xA5A5A5A5u), src(n + guard, 0xA5A5A5A5u);
  uint64_t count[2] = {~0ull, ~0ull};
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_arena, arena.data(), arena_bytes), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_conn, conn.data(), 4 * n), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_snd, snd.data(), 16 * n_conns), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_keep, keep.data(), keep.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_off, off.data(), 8 * off.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_len, ln.data(), 4 * ln.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_oc, oc.data(), 4 * oc.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_src, src.data(), 4 * src.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_count, count, 16), TCPCK_OK);
#define RESEND(CTX, M, R, A, ST, LEN, S, N, CNT, SCR)                                                                   \
  tcpck_batch_resend(CTX, M, R, A, arena_bytes, ST, LEN, nullptr, nullptr, static_cast<const uint32_t *>(d_conn),        \
                     static_cast<const tcpck_snd_state *>(S), n_conns, N, static_cast<uint8_t *>(d_keep),                \
                     static_cast<uint64_t *>(d_off), static_cast<uint32_t *>(d_len), static_cast<uint32_t *>(d_oc),      \
                     static_cast<uint32_t *>(d_src), n, static_cast<uint64_t *>(static_cast<void *>(CNT)), SCR, nullptr)
  CHECK_RC(RESEND(nullptr, 0, 0, d_arena, stride, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 3, 0, d_arena, stride, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 3, d_arena, stride, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, nullptr, stride, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride + 1, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, 30, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, 32, len, d_snd, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, nullptr, n, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, (1ull << 31) + 1, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, n, nullptr, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, n, d_count, nullptr), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, n, static_cast<uint8_t *>(d_count) + 4, d_scratch), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, n, d_count, static_cast<uint8_t *>(d_scratch) + 8), TCPCK_EINVAL);
  CHECK_RC(RESEND(ctx, 0, 0, d_arena, stride, len, d_snd, n, d_count, d_scratch), TCPCK_OK);
  CHECK_RC(tcpck_stream_sync(ctx, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, arena.data(), d_arena, arena_bytes), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, keep.data(), d_keep, keep.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, off.data(), d_off, 8 * off.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, ln.data(), d_len, 4 * ln.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, oc.data(), d_oc, 4 * oc.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, src.data(), d_src, 4 * src.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, count, d_count, 16), TCPCK_OK);
  CHECK(count[0] == total && count[1] == ~0ull);
  CHECK(arena == want_arena);
  CHECK(std::memcmp(keep.data(), want_keep.data(), n) == 0);
  CHECK(std::memcmp(off.data(), want_off.data(), 8 * total) == 0);
  CHECK(std::memcmp(ln.data(), want_len.data(), 4 * total) == 0);
  CHECK(std::memcmp(oc.data(), want_conn.data(), 4 * total) == 0);
  CHECK(std::memcmp(src.data(), want_src.data(), 4 * total) == 0);
  for (uint64_t k = n; k < keep.size(); ++k) CHECK(keep[k] == 0xA5);
  for (uint64_t j = total; j < src.size(); ++j)
    CHECK(off[j] == 0xA5A5A5A5A5A5A5A5ull && ln[j] == 0xA5A5A5A5u && oc[j] == 0xA5A5A5A5u && src[j] == 0xA5A5A5A5u);
  for (void *p : {d_arena, d_conn, d_snd, d_keep, d_off, d_len, d_oc, d_src, d_count, d_scratch})
    CHECK_RC(tcpck_device_free(ctx, p), TCPCK_OK);
  CHECK_RC(tcpck_ctx_destroy(ctx), TCPCK_OK);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "cpu";
  if (what == "cpu") {
    CHECK(argc > 2);
    queues_on_manifest(argv[2]);
    host_errors();
  } else if (what == "gpu") {
    gpu_checks();
  } else {
    std::fprintf(stderr, "usage: resend_host_test cpu <manifest> | gpu\n");
    return 2;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
