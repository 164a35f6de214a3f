// deliver_host_test.cc -- the receive delivery entry points' host logic under
// AddressSanitizer + UBSan: tcpck_plan_deliver (plain host code) and the
// argument checks and launcher arithmetic of tcpck_batch_deliver.  Linked
// against tcp-stack_amd/libtcpck_asan.so (tcp-stack_amd/Makefile `asan`; the
// device code is not sanitized); tests/test_deliver_asan.py runs it.
//
//   deliver_host_test cpu <manifest>   no device: the planner on the arrival
//       sequences of the manifest (the golden ones and seeded random ones, the
//       expected outputs from tests/deliver_np.py plan_np), every array a heap
//       block of exactly its size; every TCPCK_EINVAL path of both entry points
//   deliver_host_test gpu              device 0: tcpck_batch_deliver's checks
//       with a live context, and one small delivery checked on the host
//
// Manifest: per sequence a line
//   seq n recv_bytes rcv_nxt snd_nxt snd_una rcv_wnd consumed f_rcv_nxt f_snd_una f_rcv_wnd f_delivered
// then n lines: <64 hex digits of host-order header> ok length dst verdict ack.
// Prints "ok <n checks>" and exits 0, or names the first failed check.
#include <hip/hip_runtime_api.h>

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
#define CHECK_RC(expr, want)                                                                                     \
  do {                                                                                                           \
    ++g_checks;                                                                                                  \
    const int rc_ = (expr);                                                                                      \
    if (rc_ != (want)) {                                                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s = %d (%s), want %d\n", __FILE__, __LINE__, #expr, rc_,             \
                   tcpck_strerror(rc_), (want));                                                                 \
      std::exit(1);                                                                                              \
    }                                                                                                            \
  } while (0)

int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

void planner_on_manifest(const char *path) {
  FILE *f = std::fopen(path, "r");
  CHECK(f != nullptr);
  char word[16];
  int sequences = 0;
  while (std::fscanf(f, "%15s", word) == 1) {
    CHECK(std::strcmp(word, "seq") == 0);
    uint64_t n, recv_bytes, v[9];
    CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64, &n, &recv_bytes) == 2);
    for (auto &x : v) CHECK(std::fscanf(f, "%" SCNu64, &x) == 1);
    // exactly sized heap blocks: a read or write past any of them is a report
    std::vector<uint8_t> hdr(32 * n), ok(n), verdict(n), want_verdict(n);
    std::vector<uint32_t> lengths(n), ack(n), want_ack(n);
    std::vector<uint64_t> dst(n), want_dst(n);
    for (uint64_t k = 0; k < n; ++k) {
      char hex[65];
      uint64_t o, l, d, vd, a;
      CHECK(std::fscanf(f, "%64s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, hex, &o, &l, &d, &vd, &a) == 6);
      for (int b = 0; b < 32; ++b) hdr[32 * k + b] = static_cast<uint8_t>(hexval(hex[2 * b]) * 16 + hexval(hex[2 * b + 1]));
      ok[k] = static_cast<uint8_t>(o);
      lengths[k] = static_cast<uint32_t>(l);
      want_dst[k] = d;
      want_verdict[k] = static_cast<uint8_t>(vd);
      want_ack[k] = static_cast<uint32_t>(a);
    }
    tcpck_rcv_state st{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1]), static_cast<uint32_t>(v[2]),
                       static_cast<uint16_t>(v[3]), 0, 0};
    uint64_t consumed = ~0ull;
    CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, recv_bytes, dst.data(), verdict.data(),
                                ack.data(), &consumed),
             TCPCK_OK);
    CHECK(consumed == v[4] && st.rcv_nxt == v[5] && st.snd_una == v[6] && st.rcv_wnd == v[7] && st.delivered == v[8]);
    CHECK(st.snd_nxt == v[1]);
    CHECK(dst == want_dst && verdict == want_verdict && ack == want_ack);
    // the same walk image by image (count 1 calls) reaches the same state
    tcpck_rcv_state one{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1]), static_cast<uint32_t>(v[2]),
                        static_cast<uint16_t>(v[3]), 0, 0};
    for (uint64_t k = 0; k < v[4]; ++k) {
      uint64_t d1, c1;
      uint8_t v1;
      uint32_t a1;
      CHECK_RC(tcpck_plan_deliver(hdr.data() + 32 * k, ok.data() + k, nullptr, lengths[k], 1, &one, recv_bytes, &d1, &v1,
                                  &a1, &c1),
               TCPCK_OK);
      CHECK(c1 == 1 && d1 == want_dst[k] && v1 == want_verdict[k] && a1 == want_ack[k]);
    }
    CHECK(std::memcmp(&one, &st, sizeof one) == 0);
    ++sequences;
  }
  std::fclose(f);
  CHECK(sequences >= 3);
}

void planner_errors() {
  const uint64_t n = 3;
  std::vector<uint8_t> hdr(32 * n), ok(n, 1), verdict(n);
  std::vector<uint32_t> lengths(n, 64), ack(n);
  std::vector<uint64_t> dst(n);
  tcpck_rcv_state st{};
  uint64_t used = 0;
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, 4096, dst.data(), verdict.data(),
                              ack.data(), &used), TCPCK_OK);
  CHECK_RC(tcpck_plan_deliver(nullptr, ok.data(), lengths.data(), 0, n, &st, 4096, dst.data(), verdict.data(), ack.data(),
                              &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), nullptr, lengths.data(), 0, n, &st, 4096, dst.data(), verdict.data(),
                              ack.data(), &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, nullptr, 4096, dst.data(), verdict.data(),
                              ack.data(), &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, 4096, nullptr, verdict.data(), ack.data(),
                              &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, 4096, dst.data(), nullptr, ack.data(),
                              &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, 4096, dst.data(), verdict.data(), nullptr,
                              &used), TCPCK_EINVAL);
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &st, 4096, dst.data(), verdict.data(),
                              ack.data(), nullptr), TCPCK_EINVAL);
  for (uint32_t len : {0u, 30u, 33u, 65u})  // h_lengths NULL: `len` short or odd
    CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), nullptr, len, n, &st, 4096, dst.data(), verdict.data(), ack.data(),
                                &used), TCPCK_EINVAL);
  for (uint32_t bad : {0u, 30u, 33u}) {
    auto l2 = lengths;
    l2[n - 1] = bad;
    CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), l2.data(), 0, n, &st, 4096, dst.data(), verdict.data(), ack.data(),
                                &used), TCPCK_EINVAL);
  }
  tcpck_rcv_state full{};
  full.delivered = 5000;  // already past the capacity given
  CHECK_RC(tcpck_plan_deliver(hdr.data(), ok.data(), lengths.data(), 0, n, &full, 4096, dst.data(), verdict.data(),
                              ack.data(), &used), TCPCK_EINVAL);
  // no images: nothing but the state and the count is touched
  used = 7;
  CHECK_RC(tcpck_plan_deliver(nullptr, nullptr, nullptr, 0, 0, &st, 0, nullptr, nullptr, nullptr, &used), TCPCK_OK);
  CHECK(used == 0);
}

// tcpck_batch_deliver's checks; they come before the context is used, so `ctx`
// may be a stand-in where there is no device
void deliver_errors(tcpck_ctx *ctx) {
  alignas(16) static uint8_t buf[256];
  const uint64_t *d64 = reinterpret_cast<const uint64_t *>(buf);
  const uint32_t *d32 = reinterpret_cast<const uint32_t *>(buf);
  CHECK_RC(tcpck_batch_deliver(nullptr, buf, 64, 64, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, nullptr, 64, 64, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 64, nullptr, nullptr, 1, nullptr, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 64, nullptr, nullptr, 1, d64, nullptr, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf + 1, 64, 64, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  for (int mis : {2, 4, 8, 15})  // d_recv not 16-B aligned
    CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 64, nullptr, nullptr, 1, d64, buf + 128 + mis, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 65, 64, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 63, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 30, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 62, 64, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 0, 0, nullptr, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 1ull << 40, 64, nullptr, nullptr, 1ull << 30, d64, buf + 128, 64, nullptr),
           TCPCK_EINVAL);  // count * stride overflows
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 0, 0, d64, nullptr, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_deliver(ctx, buf, 64, 64, nullptr, d32, 1, d64, buf + 128, 64, nullptr), TCPCK_EINVAL);
  // nothing to do: no device call either
  CHECK_RC(tcpck_batch_deliver(ctx, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr), TCPCK_OK);
}

void gpu_checks() {
  tcpck_ctx *ctx = nullptr;
  CHECK_RC(tcpck_ctx_create(0, &ctx), TCPCK_OK);
  deliver_errors(ctx);
  // 300 images in 256-B slots, lengths 32..190, every third skipped, one odd
  // dst, one past the end; destinations back to back from byte 6
  const uint64_t n = 300, stride = 256, recv_bytes = 40000;
  std::mt19937_64 rng(5);
  std::vector<uint8_t> arena(n * stride), recv(recv_bytes, 0xA5);
  for (auto &b : arena) b = static_cast<uint8_t>(rng());
  std::vector<uint64_t> off(n), dst(n);
  std::vector<uint32_t> len(n);
  uint64_t at = 6;
  for (uint64_t k = 0; k < n; ++k) {
    off[k] = k * stride + 2 * (k % 8);
    len[k] = 32 + 2 * static_cast<uint32_t>(rng() % 80);
    dst[k] = k % 3 == 2 ? TCPCK_DELIVER_SKIP : at;
    if (k == 100) dst[k] = at + 1;
    if (k == 200) dst[k] = recv_bytes - 2, len[k] = 36;
    if (dst[k] == at) at += len[k] - 32;
  }
  auto want = recv;
  for (uint64_t k = 0; k < n; ++k)
    if (dst[k] != TCPCK_DELIVER_SKIP && !(dst[k] & 1) && dst[k] + len[k] - 32 <= recv_bytes)
      std::memcpy(want.data() + dst[k], arena.data() + off[k] + 32, len[k] - 32);
  void *d_arena, *d_recv, *d_off, *d_len, *d_dst;
  CHECK_RC(tcpck_device_alloc(ctx, arena.size(), &d_arena), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, recv.size(), &d_recv), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, n * 8, &d_off), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, n * 4, &d_len), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, n * 8, &d_dst), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_arena, arena.data(), arena.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_recv, recv.data(), recv.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_off, off.data(), n * 8), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_len, len.data(), n * 4), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_dst, dst.data(), n * 8), TCPCK_OK);
  CHECK_RC(tcpck_batch_deliver(ctx, d_arena, 0, 0, static_cast<uint64_t *>(d_off), static_cast<uint32_t *>(d_len), n,
                               static_cast<uint64_t *>(d_dst), d_recv, recv_bytes, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_stream_sync(ctx, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, recv.data(), d_recv, recv.size()), TCPCK_OK);
  CHECK(recv == want);
  for (void *p : {d_arena, d_recv, d_off, d_len, d_dst}) CHECK_RC(tcpck_device_free(ctx, p), TCPCK_OK);
  CHECK_RC(tcpck_ctx_destroy(ctx), TCPCK_OK);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "cpu";
  if (what == "cpu") {
    CHECK(argc > 2);
    planner_on_manifest(argv[2]);
    planner_errors();
    alignas(16) static uint8_t stand_in[64];
    deliver_errors(reinterpret_cast<tcpck_ctx *>(stand_in));
  } else if (what == "gpu") {
    gpu_checks();
  } else {
    std::fprintf(stderr, "usage: deliver_host_test cpu <manifest> | gpu\n");
    return 2;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
