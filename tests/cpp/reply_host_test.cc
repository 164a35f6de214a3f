// reply_host_test.cc -- the batched reply builder's host code under
// AddressSanitizer + UBSan: tcpck_build_replies (plain host code) and the
// argument checks of tcpck_batch_reply / tcpck_reply_scratch_bytes.  Linked
// against tcp-stack_amd/libtcpck_asan.so (tcp-stack_amd/Makefile `asan`; the
// device code is not sanitized); tests/test_reply_asan.py runs it.
//
//   reply_host_test cpu <manifest>   no device: tcpck_build_replies on the rings
//       of the manifest (expected bytes from tests/reply_np.py), every array a
//       heap block of exactly its size; every TCPCK_EINVAL path
//   reply_host_test gpu              device 0: one small tcpck_batch_reply,
//       checked against tcpck_build_replies
//
// Manifest: per ring a line `ring n n_conns has_conn cap mode total`, then n
// lines `verdict ack conn`, n_conns lines of 64 hex digits (the templates), and
// min(total, cap) lines `<64 hex digits of reply> src`.
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

int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

void read_hex32(FILE *f, uint8_t *out) {
  char hex[80];
  CHECK(std::fscanf(f, "%64s", hex) == 1 && std::strlen(hex) == 64);
  for (int i = 0; i < 32; ++i) out[i] = static_cast<uint8_t>(hexval(hex[2 * i]) << 4 | hexval(hex[2 * i + 1]));
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

void rings_on_manifest(const char *path) {
  FILE *f = std::fopen(path, "r");
  CHECK(f != nullptr);
  char word[16];
  int rings = 0;
  while (std::fscanf(f, "%15s", word) == 1) {
    CHECK(std::strcmp(word, "ring") == 0);
    uint64_t n, n_conns, has_conn, cap, mode, total;
    CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &n, &n_conns, &has_conn,
                      &cap, &mode, &total) == 6);
    uint8_t *verdict = block<uint8_t>(n);
    uint32_t *ack = block<uint32_t>(4 * n), *conn = has_conn ? block<uint32_t>(4 * n) : nullptr;
    for (uint64_t k = 0; k < n; ++k) {
      uint64_t v, a, c;
      CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &v, &a, &c) == 3);
      verdict[k] = static_cast<uint8_t>(v), ack[k] = static_cast<uint32_t>(a);
      if (conn) conn[k] = static_cast<uint32_t>(c);
    }
    uint8_t *tmpl = block<uint8_t>(32 * n_conns);
    for (uint64_t c = 0; c < n_conns; ++c) read_hex32(f, tmpl + 32 * c);
    const uint64_t written = std::min(total, cap);
    std::vector<uint8_t> want(32 * written);
    std::vector<uint32_t> want_src(written);
    for (uint64_t j = 0; j < written; ++j) {
      read_hex32(f, want.data() + 32 * j);
      uint64_t s;
      CHECK(std::fscanf(f, "%" SCNu64, &s) == 1);
      want_src[j] = static_cast<uint32_t>(s);
    }
    // the outputs hold exactly what may be written: one byte more would be a sanitizer report
    uint8_t *replies = block<uint8_t>(32 * written);
    uint32_t *src = block<uint32_t>(4 * written);
    uint8_t dummy[16] __attribute__((aligned(16)));
    uint64_t got = 99;
    CHECK_RC(tcpck_build_replies(static_cast<int>(mode), verdict, ack, conn, tmpl, static_cast<uint32_t>(n_conns), n,
                                 replies ? replies : dummy, cap, src, &got),
             TCPCK_OK);
    CHECK(got == total);
    CHECK(written == 0 || std::memcmp(replies, want.data(), 32 * written) == 0);
    CHECK(written == 0 || std::memcmp(src, want_src.data(), 4 * written) == 0);
    // and without the source array
    if (replies) std::memset(replies, 0, 32 * written);
    CHECK_RC(tcpck_build_replies(static_cast<int>(mode), verdict, ack, conn, tmpl, static_cast<uint32_t>(n_conns), n,
                                 replies ? replies : dummy, cap, nullptr, &got),
             TCPCK_OK);
    CHECK(got == total && (written == 0 || std::memcmp(replies, want.data(), 32 * written) == 0));
    std::free(verdict), std::free(ack), std::free(conn), std::free(tmpl), std::free(replies), std::free(src);
    ++rings;
  }
  std::fclose(f);
  CHECK(rings >= 6);
}

void host_errors() {
  const uint64_t n = 40;
  uint8_t *verdict = block<uint8_t>(n);
  uint32_t *ack = block<uint32_t>(4 * n), *conn = block<uint32_t>(4 * n), *src = block<uint32_t>(4 * n + 4);
  uint8_t *tmpl = block<uint8_t>(32 * 3 + 16), *replies = block<uint8_t>(32 * n + 16);
  uint64_t *total = block<uint64_t>(16);
  for (uint64_t k = 0; k < n; ++k) verdict[k] = k % 3 ? TCPCK_RCV_SEND_ACK : TCPCK_RCV_RST, conn[k] = k % 3, ack[k] = 7;
  const auto untouched = [&] {
    for (uint64_t i = 0; i < 32 * n + 16; ++i) CHECK(replies[i] == 0x5A);
    for (uint64_t i = 0; i <= n; ++i) CHECK(src[i] == 0x5A5A5A5Au);
    CHECK(total[0] == 0x5A5A5A5A5A5A5A5Aull && total[1] == total[0]);
  };
  const auto bytes = [](auto *p, size_t by) { return reinterpret_cast<uint8_t *>(p) + by; };
#define BUILD(M, V, A, C, T, NC, N, R, CAP, S, TOT) \
  tcpck_build_replies(M, V, A, C, T, NC, N, R, CAP, S, TOT)
  CHECK_RC(BUILD(2, verdict, ack, conn, tmpl, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(-1, verdict, ack, conn, tmpl, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, (1ull << 31) + 1, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, nullptr, ack, conn, tmpl, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, nullptr, conn, tmpl, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, n, nullptr, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, n, replies, n, src, nullptr), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, nullptr, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, reinterpret_cast<uint32_t *>(bytes(ack, 2)), conn, tmpl, 3, n - 1, replies, n, src, total),
           TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, reinterpret_cast<uint32_t *>(bytes(conn, 1)), tmpl, 3, n - 1, replies, n, src, total),
           TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, n, replies, n, reinterpret_cast<uint32_t *>(bytes(src, 2)), total),
           TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl + 8, 3, n, replies, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, n, replies + 4, n, src, total), TCPCK_EINVAL);
  CHECK_RC(BUILD(0, verdict, ack, conn, tmpl, 3, n, replies, n, src, reinterpret_cast<uint64_t *>(bytes(total, 4))),
           TCPCK_EINVAL);
  untouched();
  // nothing to do: only the count is written
  CHECK_RC(BUILD(1, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, total + 1), TCPCK_OK);
  CHECK(total[1] == 0);
  total[1] = total[0];
  CHECK_RC(BUILD(1, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr), TCPCK_OK);
  untouched();
  // the alignments that are enough
  CHECK_RC(BUILD(0, verdict, ack + 1, conn + 1, tmpl + 16, 2, n - 1, replies + 16, n - 1, src + 1, total + 1), TCPCK_OK);
  CHECK(total[1] > 10 && total[1] < n && src[0] == 0x5A5A5A5Au && replies[15] == 0x5A);
  uint64_t bytes_out = 5;
  CHECK_RC(tcpck_reply_scratch_bytes((1ull << 31) + 1, &bytes_out), TCPCK_EINVAL);
  CHECK_RC(tcpck_reply_scratch_bytes(8, nullptr), TCPCK_EINVAL);
  CHECK(bytes_out == 5);
  size_t small = 0, large = 0;
  CHECK_RC(tcpck_reply_scratch_bytes(0, &small), TCPCK_OK);
  CHECK_RC(tcpck_reply_scratch_bytes(1ull << 31, &large), TCPCK_OK);
  CHECK(small >= 16 && small % 16 == 0 && large % 16 == 0 && large > small);
  std::free(verdict), std::free(ack), std::free(conn), std::free(src), std::free(tmpl), std::free(replies), std::free(total);
}

void gpu_checks() {
  tcpck_ctx *ctx = nullptr;
  CHECK_RC(tcpck_ctx_create(0, &ctx), TCPCK_OK);
  const uint64_t n = 3000, guard = 16;
  const uint32_t n_conns = 5;
  std::mt19937_64 rng(11);
  std::vector<uint8_t> verdict(n), tmpl(32 * n_conns);
  std::vector<uint32_t> ack(n), conn(n);
  for (auto &b : tmpl) b = static_cast<uint8_t>(rng());
  const uint8_t kinds[] = {0, 1, 7, 5, 12, TCPCK_RCV_RST, TCPCK_RCV_HOST, 4};
  for (uint64_t k = 0; k < n; ++k) {
    verdict[k] = kinds[rng() % 8];
    ack[k] = static_cast<uint32_t>(rng());
    conn[k] = rng() % 10 == 0 ? TCPCK_CONN_NONE : static_cast<uint32_t>(rng() % (n_conns + 1));
  }
  std::vector<uint32_t> want_src(n);
  uint64_t total = 0;
  uint8_t *wp = block<uint8_t>(32 * n);  // (16-B aligned)
  uint8_t *tp = block<uint8_t>(32 * n_conns);
  std::memcpy(tp, tmpl.data(), tmpl.size());
  CHECK_RC(tcpck_build_replies(0, verdict.data(), ack.data(), conn.data(), tp, n_conns, n, wp, n, want_src.data(), &total),
           TCPCK_OK);
  CHECK(total > n / 4 && total < n);
  size_t scratch_bytes = 0;
  CHECK_RC(tcpck_reply_scratch_bytes(n, &scratch_bytes), TCPCK_OK);
  void *d_verdict, *d_ack, *d_conn, *d_tmpl, *d_replies, *d_src, *d_count, *d_scratch;
  CHECK_RC(tcpck_device_alloc(ctx, n, &d_verdict), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * n, &d_ack), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * n, &d_conn), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 32 * n_conns, &d_tmpl), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 32 * (n + guard), &d_replies), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * (n + guard), &d_src), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 16, &d_count), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, scratch_bytes, &d_scratch), TCPCK_OK);
  std::vector<uint8_t> replies(32 * (n + guard), 0xA5);
  std::vector<uint32_t> src(n + guard, 0xA5A5A5A5u);
  uint64_t count[2] = {~0ull, ~0ull};
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_verdict, verdict.data(), n), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_ack, ack.data(), 4 * n), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_conn, conn.data(), 4 * n), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_tmpl, tmpl.data(), tmpl.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_replies, replies.data(), replies.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_src, src.data(), 4 * src.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_count, count, 16), TCPCK_OK);
#define REPLY(CTX, M, V, A, T, N, R, CNT, SCR)                                                                      \
  tcpck_batch_reply(CTX, M, static_cast<const uint8_t *>(V), static_cast<const uint32_t *>(A),                      \
                    static_cast<const uint32_t *>(d_conn), T, n_conns, N, R, n, static_cast<uint32_t *>(d_src), \
                    static_cast<uint64_t *>(static_cast<void *>(CNT)), SCR, nullptr)
  CHECK_RC(REPLY(nullptr, 0, d_verdict, d_ack, d_tmpl, n, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 3, d_verdict, d_ack, d_tmpl, n, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, nullptr, d_ack, d_tmpl, n, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, nullptr, d_tmpl, n, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, nullptr, n, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, (1ull << 31) + 1, d_replies, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, nullptr, d_count, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, d_replies, nullptr, d_scratch), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, d_replies, d_count, nullptr), TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, static_cast<uint8_t *>(d_replies) + 8, d_count, d_scratch),
           TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, d_replies, static_cast<uint8_t *>(d_count) + 4, d_scratch),
           TCPCK_EINVAL);
  CHECK_RC(REPLY(ctx, 0, d_verdict, d_ack, d_tmpl, n, d_replies, d_count, d_scratch), TCPCK_OK);
  CHECK_RC(tcpck_stream_sync(ctx, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, replies.data(), d_replies, replies.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, src.data(), d_src, 4 * src.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, count, d_count, 16), TCPCK_OK);
  CHECK(count[0] == total && count[1] == ~0ull);
  CHECK(std::memcmp(replies.data(), wp, 32 * total) == 0);
  CHECK(std::memcmp(src.data(), want_src.data(), 4 * total) == 0);
  for (uint64_t i = 32 * total; i < replies.size(); ++i) CHECK(replies[i] == 0xA5);
  for (uint64_t j = total; j < src.size(); ++j) CHECK(src[j] == 0xA5A5A5A5u);
  for (void *p : {d_verdict, d_ack, d_conn, d_tmpl, d_replies, d_src, d_count, d_scratch})
    CHECK_RC(tcpck_device_free(ctx, p), TCPCK_OK);
  CHECK_RC(tcpck_ctx_destroy(ctx), TCPCK_OK);
  std::free(wp), std::free(tp);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "cpu";
  if (what == "cpu") {
    CHECK(argc > 2);
    rings_on_manifest(argv[2]);
    host_errors();
  } else if (what == "gpu") {
    gpu_checks();
  } else {
    std::fprintf(stderr, "usage: reply_host_test cpu <manifest> | gpu\n");
    return 2;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
