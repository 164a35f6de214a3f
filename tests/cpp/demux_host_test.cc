// demux_host_test.cc -- the receive demultiplexer's host logic under
// AddressSanitizer + UBSan: the connection table's mirror and image rebuild
// (tcpck_conn_table_*), tcpck_plan_deliver_multi (plain host code) and the
// argument checks of tcpck_batch_demux.  Linked against
// tcp-stack_amd/libtcpck_asan.so (tcp-stack_amd/Makefile `asan`; the device
// code is not sanitized); tests/test_demux_asan.py runs it.
//
//   demux_host_test cpu <manifest>   no device: a seeded churn of a host-only
//       table against a std::map; the multi planner on the rings of the
//       manifest (expected outputs from tests/demux_np.py plan_multi_np), every
//       array a heap block of exactly its size; every TCPCK_EINVAL path
//   demux_host_test gpu              device 0: create / commit / demux /
//       destroy on one small table, checked against tcpck_conn_table_find
//
// Manifest: per ring a line `ring n n_conns`, then n_conns lines
//   rcv_nxt snd_nxt snd_una rcv_wnd delivered recv_base recv_bytes flags
//   f_rcv_nxt f_snd_una f_rcv_wnd f_delivered f_stopped_at
// then n lines: <64 hex digits of host-order header> ok length conn dst verdict ack.
// Prints "ok <n checks>" and exits 0, or names the first failed check.
#include <hip/hip_runtime_api.h>

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <tuple>
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

using Key = std::tuple<uint16_t, uint32_t, uint16_t>;

Key nth_key(uint32_t i) {  // clustered: consecutive ports and addresses, three listeners
  if (i < 3) return Key(static_cast<uint16_t>(80 + i), 0, 0);
  return Key(static_cast<uint16_t>(80 + i % 3), 0x0A000000u + i / 6, static_cast<uint16_t>(4000 + i % 6));
}

void table_churn() {
  for (uint32_t max_conns : {1u, 31u, 128u}) {
    tcpck_conn_table *t = nullptr;
    CHECK_RC(tcpck_conn_table_create(nullptr, max_conns, &t), TCPCK_OK);
    std::map<Key, uint32_t> want;
    std::mt19937_64 rng(max_conns);
    const uint32_t n_keys = 3 * max_conns + 3;
    for (int step = 0; step < 5000; ++step) {
      const Key key = nth_key(static_cast<uint32_t>(rng() % n_keys));
      const auto [hp, ip, pp] = key;
      const uint64_t r = rng() % 10;
      if (r < 5) {
        const uint32_t id = static_cast<uint32_t>(rng() % UINT32_MAX);
        if (want.count(key) || want.size() < max_conns) {
          CHECK_RC(tcpck_conn_table_set(t, hp, ip, pp, id), TCPCK_OK);
          want[key] = id;
        } else {
          CHECK_RC(tcpck_conn_table_set(t, hp, ip, pp, id), TCPCK_ENOMEM);
        }
      } else if (r < 8) {
        CHECK_RC(tcpck_conn_table_erase(t, hp, ip, pp), TCPCK_OK);
        want.erase(key);
      }
      uint32_t got = 0;
      CHECK_RC(tcpck_conn_table_find(t, hp, ip, pp, &got), TCPCK_OK);
      CHECK(got == (want.count(key) ? want[key] : TCPCK_CONN_NONE));
      if (step % 250 == 249) {
        for (uint32_t i = 0; i < n_keys; ++i) {
          const auto [a, b, c] = nth_key(i);
          CHECK_RC(tcpck_conn_table_find(t, a, b, c, &got), TCPCK_OK);
          CHECK(got == (want.count(nth_key(i)) ? want[nth_key(i)] : TCPCK_CONN_NONE));
        }
        uint64_t slots = 0, entries = 0, wrapped = 0;
        uint32_t longest = 0;
        CHECK_RC(tcpck_conn_table_commit(t, nullptr), TCPCK_OK);
        CHECK_RC(tcpck_conn_table_stats(t, &slots, &entries, &longest, &wrapped), TCPCK_OK);
        CHECK(slots >= 64 && slots >= 2 * max_conns && (slots & (slots - 1)) == 0 && entries == want.size());
        CHECK(longest <= entries && wrapped <= entries && (entries == 0) == (longest == 0));
      }
    }
    CHECK_RC(tcpck_conn_table_destroy(t), TCPCK_OK);
  }
}

void table_errors() {
  tcpck_conn_table *t = nullptr;
  uint32_t id = 5;
  CHECK_RC(tcpck_conn_table_create(nullptr, 0, &t), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_create(nullptr, (1u << 22) + 1, &t), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_create(nullptr, 8, nullptr), TCPCK_EINVAL);
  CHECK(t == nullptr);
  CHECK_RC(tcpck_conn_table_set(nullptr, 1, 1, 1, 1), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_erase(nullptr, 1, 1, 1), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_find(nullptr, 1, 1, 1, &id), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_commit(nullptr, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_stats(nullptr, nullptr, nullptr, nullptr, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_destroy(nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_create(nullptr, 8, &t), TCPCK_OK);
  CHECK_RC(tcpck_conn_table_set(t, 1, 1, 1, TCPCK_CONN_NONE), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_find(t, 1, 1, 1, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_find(t, 1, 1, 1, &id), TCPCK_OK);
  CHECK(id == TCPCK_CONN_NONE);
  CHECK_RC(tcpck_conn_table_stats(t, nullptr, nullptr, nullptr, nullptr), TCPCK_OK);
  // tcpck_batch_demux's checks that need no device: a host-only table is refused
  alignas(16) static uint8_t buf[256];
  alignas(16) static uint8_t stand_in[64];
  tcpck_ctx *ctx = reinterpret_cast<tcpck_ctx *>(stand_in);
  uint32_t *d32 = reinterpret_cast<uint32_t *>(buf + 128);
  CHECK_RC(tcpck_conn_table_commit(t, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_batch_demux(nullptr, t, buf, 1, d32, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, nullptr, buf, 1, d32, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, buf, 1, d32, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, buf, 0, d32, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_conn_table_destroy(t), TCPCK_OK);
}

struct Ring {
  std::vector<uint8_t> hdr, ok, verdict;
  std::vector<uint32_t> lengths, conn, ack;
  std::vector<uint64_t> dst;
  std::vector<tcpck_conn_state> conns;
};

void planner_on_manifest(const char *path) {
  FILE *f = std::fopen(path, "r");
  CHECK(f != nullptr);
  char word[16];
  int rings = 0;
  while (std::fscanf(f, "%15s", word) == 1) {
    CHECK(std::strcmp(word, "ring") == 0);
    uint64_t n, n_conns;
    CHECK(std::fscanf(f, "%" SCNu64 " %" SCNu64, &n, &n_conns) == 2);
    // exactly sized heap blocks: a read or write past any of them is a report
    Ring r;
    r.conns.resize(n_conns);
    std::vector<tcpck_conn_state> want_conns(n_conns);
    for (uint64_t c = 0; c < n_conns; ++c) {
      uint64_t v[13];
      for (auto &x : v) CHECK(std::fscanf(f, "%" SCNu64, &x) == 1);
      tcpck_conn_state s{};
      s.rcv = tcpck_rcv_state{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1]), static_cast<uint32_t>(v[2]),
                              static_cast<uint16_t>(v[3]), 0, v[4]};
      s.recv_base = v[5], s.recv_bytes = v[6], s.flags = static_cast<uint32_t>(v[7]);
      s.stopped_at = 99;  // output only
      r.conns[c] = s;
      s.rcv.rcv_nxt = static_cast<uint32_t>(v[8]), s.rcv.snd_una = static_cast<uint32_t>(v[9]);
      s.rcv.rcv_wnd = static_cast<uint16_t>(v[10]), s.rcv.delivered = v[11], s.stopped_at = v[12];
      want_conns[c] = s;
    }
    r.hdr.resize(32 * n), r.ok.resize(n), r.verdict.resize(n), r.lengths.resize(n), r.conn.resize(n);
    r.ack.resize(n), r.dst.resize(n);
    std::vector<uint8_t> want_verdict(n);
    std::vector<uint32_t> want_ack(n);
    std::vector<uint64_t> want_dst(n);
    for (uint64_t k = 0; k < n; ++k) {
      char hex[65];
      uint64_t o, l, c, d, vd, a;
      CHECK(std::fscanf(f, "%64s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, hex, &o, &l, &c, &d,
                        &vd, &a) == 7);
      for (int b = 0; b < 32; ++b)
        r.hdr[32 * k + b] = static_cast<uint8_t>(hexval(hex[2 * b]) * 16 + hexval(hex[2 * b + 1]));
      r.ok[k] = static_cast<uint8_t>(o);
      r.lengths[k] = static_cast<uint32_t>(l);
      r.conn[k] = static_cast<uint32_t>(c);
      want_dst[k] = d;
      want_verdict[k] = static_cast<uint8_t>(vd);
      want_ack[k] = static_cast<uint32_t>(a);
    }
    CHECK_RC(tcpck_plan_deliver_multi(r.hdr.data(), r.ok.data(), r.conn.data(), r.lengths.data(), 0, n, r.conns.data(),
                                      static_cast<uint32_t>(n_conns), r.dst.data(), r.verdict.data(), r.ack.data()),
             TCPCK_OK);
    CHECK(r.dst == want_dst && r.verdict == want_verdict && r.ack == want_ack);
    for (uint64_t c = 0; c < n_conns; ++c) CHECK(std::memcmp(&r.conns[c], &want_conns[c], sizeof(tcpck_conn_state)) == 0);
    ++rings;
  }
  std::fclose(f);
  CHECK(rings >= 3);
}

void planner_errors() {
  const uint64_t n = 4;
  std::vector<uint8_t> hdr(32 * n), ok(n, 1), verdict(n, 0x5A);
  std::vector<uint32_t> lengths(n, 64), conn{0, 1, TCPCK_CONN_NONE, 1}, ack(n, 0x5A5A);
  std::vector<uint64_t> dst(n, 0x5A5A);
  auto fresh = [] {
    std::vector<tcpck_conn_state> c(2);
    for (size_t i = 0; i < 2; ++i) {
      c[i] = tcpck_conn_state{};
      c[i].recv_base = 4096 * i, c[i].recv_bytes = 4000, c[i].stopped_at = 99;
    }
    return c;
  };
  auto untouched = [&](const std::vector<tcpck_conn_state> &c) {
    for (uint64_t k = 0; k < n; ++k) CHECK(dst[k] == 0x5A5A && verdict[k] == 0x5A && ack[k] == 0x5A5A);
    for (const auto &s : c) CHECK(s.stopped_at == 99);
  };
  auto c = fresh();
#define MULTI(H, O, C, L, LEN, CS, NC, D, V, A) \
  tcpck_plan_deliver_multi(H, O, C, L, LEN, n, CS, NC, D, V, A)
  CHECK_RC(MULTI(nullptr, ok.data(), conn.data(), lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), nullptr, conn.data(), lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), ok.data(), nullptr, lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, nullptr, 2, dst.data(), verdict.data(), ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, c.data(), 2, nullptr, verdict.data(), ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, c.data(), 2, dst.data(), nullptr, ack.data()),
           TCPCK_EINVAL);
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), nullptr),
           TCPCK_EINVAL);
  for (uint32_t len : {0u, 30u, 33u, 65u})  // h_lengths NULL: `len` short or odd
    CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), nullptr, len, c.data(), 2, dst.data(), verdict.data(), ack.data()),
             TCPCK_EINVAL);
  for (uint32_t bad : {0u, 30u, 33u}) {
    auto l2 = lengths;
    l2[n - 1] = bad;
    CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), l2.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
             TCPCK_EINVAL);
  }
  for (uint32_t bad : {2u, 3u, TCPCK_CONN_NONE - 1}) {  // neither NONE nor below n_conns
    auto c2 = conn;
    c2[n - 1] = bad;
    CHECK_RC(MULTI(hdr.data(), ok.data(), c2.data(), lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
             TCPCK_EINVAL);
  }
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, c.data(), 1, dst.data(), verdict.data(), ack.data()),
           TCPCK_EINVAL);
  untouched(c);
  for (int which = 0; which < 4; ++which) {
    auto b = fresh();
    if (which == 0) b[1].recv_base = 4097;                 // odd
    if (which == 1) b[1].recv_base = UINT64_MAX - 1;       // base + bytes overflows
    if (which == 2) b[1].recv_bytes = UINT64_MAX - 4095;
    if (which == 3) b[1].rcv.delivered = 4001;             // already past the window
    CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, b.data(), 2, dst.data(), verdict.data(), ack.data()),
             TCPCK_EINVAL);
    untouched(b);
  }
  CHECK_RC(MULTI(hdr.data(), ok.data(), conn.data(), lengths.data(), 0, c.data(), 2, dst.data(), verdict.data(), ack.data()),
           TCPCK_OK);
  CHECK(c[0].stopped_at == TCPCK_NOT_STOPPED && verdict[2] == TCPCK_RCV_RST);
#undef MULTI
  // no images: only stopped_at is touched; no connections either: nothing is
  CHECK_RC(tcpck_plan_deliver_multi(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr),
           TCPCK_OK);
  auto d = fresh();
  CHECK_RC(tcpck_plan_deliver_multi(nullptr, nullptr, nullptr, nullptr, 0, 0, d.data(), 2, nullptr, nullptr, nullptr),
           TCPCK_OK);
  CHECK(d[1].stopped_at == TCPCK_NOT_STOPPED);
}

void gpu_checks() {
  tcpck_ctx *ctx = nullptr;
  CHECK_RC(tcpck_ctx_create(0, &ctx), TCPCK_OK);
  tcpck_conn_table *t = nullptr;
  CHECK_RC(tcpck_conn_table_create(ctx, 100, &t), TCPCK_OK);
  const uint64_t n = 300;
  void *d_hdr, *d_conn;
  CHECK_RC(tcpck_device_alloc(ctx, 32 * n, &d_hdr), TCPCK_OK);
  CHECK_RC(tcpck_device_alloc(ctx, 4 * (n + 16), &d_conn), TCPCK_OK);
  // never committed: refused, whatever else is right
  CHECK_RC(tcpck_batch_demux(ctx, t, d_hdr, n, static_cast<uint32_t *>(d_conn), nullptr), TCPCK_EINVAL);
  for (uint32_t i = 0; i < 100; i += 2) {  // every second key of the cluster
    const auto [hp, ip, pp] = nth_key(i);
    CHECK_RC(tcpck_conn_table_set(t, hp, ip, pp, 1000 + i), TCPCK_OK);
  }
  CHECK_RC(tcpck_conn_table_commit(t, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_batch_demux(ctx, t, nullptr, n, static_cast<uint32_t *>(d_conn), nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, d_hdr, n, nullptr, nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, static_cast<uint8_t *>(d_hdr) + 2, n - 1, static_cast<uint32_t *>(d_conn), nullptr),
           TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, d_hdr, n,
                             reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_conn) + 2), nullptr), TCPCK_EINVAL);
  CHECK_RC(tcpck_batch_demux(ctx, t, nullptr, 0, nullptr, nullptr), TCPCK_OK);
  std::mt19937_64 rng(9);
  std::vector<uint8_t> hdr(32 * n);
  std::vector<uint32_t> conn(n + 16, 0xA5A5A5A5u), want(n);
  for (auto &b : hdr) b = static_cast<uint8_t>(rng());
  for (uint64_t k = 0; k < n; ++k) {
    const auto [hp, ip, pp] = nth_key(static_cast<uint32_t>(rng() % 100));
    uint8_t *h = hdr.data() + 32 * k;
    std::memcpy(h, &ip, 4);
    std::memcpy(h + 12, &pp, 2);
    std::memcpy(h + 14, &hp, 2);
    const bool syn = rng() % 4 == 0;  // SYN without ACK: the listener's key
    h[25] = static_cast<uint8_t>((h[25] & ~0x48) | (syn ? 0x40 : (rng() % 2 ? 0x08 : 0x48)));
    CHECK_RC(tcpck_conn_table_find(t, hp, syn ? 0 : ip, syn ? 0 : pp, &want[k]), TCPCK_OK);
  }
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_hdr, hdr.data(), hdr.size()), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_h2d(ctx, d_conn, conn.data(), 4 * conn.size()), TCPCK_OK);
  CHECK_RC(tcpck_batch_demux(ctx, t, d_hdr, n, static_cast<uint32_t *>(d_conn), nullptr), TCPCK_OK);
  CHECK_RC(tcpck_stream_sync(ctx, nullptr), TCPCK_OK);
  CHECK_RC(tcpck_memcpy_d2h(ctx, conn.data(), d_conn, 4 * conn.size()), TCPCK_OK);
  uint64_t hits = 0;
  for (uint64_t k = 0; k < n; ++k) {
    CHECK(conn[k] == want[k]);
    hits += want[k] != TCPCK_CONN_NONE;
  }
  CHECK(hits > 50 && hits < n - 50);
  for (uint64_t k = n; k < n + 16; ++k) CHECK(conn[k] == 0xA5A5A5A5u);
  CHECK_RC(tcpck_device_free(ctx, d_hdr), TCPCK_OK);
  CHECK_RC(tcpck_device_free(ctx, d_conn), TCPCK_OK);
  CHECK_RC(tcpck_conn_table_destroy(t), TCPCK_OK);
  CHECK_RC(tcpck_ctx_destroy(ctx), TCPCK_OK);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "cpu";
  if (what == "cpu") {
    CHECK(argc > 2);
    table_churn();
    table_errors();
    planner_on_manifest(argv[2]);
    planner_errors();
  } else if (what == "gpu") {
    gpu_checks();
  } else {
    std::fprintf(stderr, "usage: demux_host_test cpu <manifest> | gpu\n");
    return 2;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
