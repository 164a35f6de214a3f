// tests/golden/gen_reply.cc -- generates the committed reply fixtures
// (reply_golden.bin + reply_golden.json): the 32-byte ACK and RST datagrams the
// REFERENCE builds, made with its own inline helpers:
//
//   ACK  SocketInternal::SendAck (socket-internal.h:293-299): MakeTcpPacket(0),
//        AckHeader(seq, ack, wnd); SocketInternal::SendPacket
//        (src/socket-internal.cc:35-42): SetSource, SetDestination,
//        TcpHeaderH2N; SocketManager::SendPacket (src/socket-manager.cc:9-10),
//        RESTATED here: Checksum() = 0; Checksum() = CalculateChecksum(*p)
//   RST  SocketManager::ReceivePacket (socket-manager.h:201-207):
//        MakeTcpPacket(0), RstHeader(const TcpHeader &, ...), TcpHeaderH2N, the
//        same two checksum lines -- and no SetSource / SetDestination
//
// The zeroed heap.  TcpPacket's constructor placement-news a TcpHeader into a
// `new char[]` buffer (tcp-header.h:270-273): default-initialisation, so every
// header byte the helpers do not set -- 8-11, 24, the other bits of 25, 30-31,
// and in an RST the addresses, ports, ack and window too -- is whatever the
// heap held.  The library defines those bytes (an ACK takes them from the
// connection's template, an RST has them zero), so this translation unit
// replaces global operator new[] with a zeroing one: the fixture is then what
// the reference sends from a fresh heap, and a template that is zero outside
// its set fields reproduces it exactly.  The program exits non-zero if any
// unset byte of any image is not 0.
//
// Built and run only in the build container, where /root/reference exists:
//     sh tests/golden/make_reply_golden.sh
// The reference header is #included by path; no reference source is copied.
// Output = data only: per case its inputs (JSON) and its 32 bytes (blob).
#include "socket-internal.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

void *operator new[](std::size_t n) {
  void *p = std::calloc(n ? n : 1, 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { std::free(p); }

using namespace tcp_stack;

namespace {

uint64_t rng = 0xD1B54A32D192ED03ull;  // fixed seed
uint32_t next32() {
  rng ^= rng << 13;
  rng ^= rng >> 7;
  rng ^= rng << 17;
  return static_cast<uint32_t>(rng >> 32);
}

struct Case {
  bool rst;
  const char *group;
  uint32_t seq, ack;  // RST: ack = the answered packet's acknowledgement number, seq unused
  uint16_t wnd;
  uint32_t src_ip, dst_ip;
  uint16_t src_port, dst_port;
  uint8_t image[32];
  uint32_t word_sum;  // of the image with a zero checksum field
};

void build(Case &c) {
  auto p = MakeTcpPacket(0);
  if (!c.rst) {
    AckHeader(c.seq, c.ack, c.wnd, &p->GetHeader());       // SendAck
    SetSource(c.src_ip, c.src_port, &p->GetHeader());       // SocketInternal::SendPacket
    SetDestination(c.dst_ip, c.dst_port, &p->GetHeader());
  } else {
    TcpHeader answered = TcpHeader();
    answered.AcknowledgementNumber() = c.ack;
    RstHeader(answered, &p->GetHeader());                   // ReceivePacket, no socket
  }
  TcpHeaderH2N(p->GetHeader());
  p->GetHeader().Checksum() = 0;                            // src/socket-manager.cc:9-10
  c.word_sum = static_cast<uint16_t>(~CalculateChecksum(*p));
  p->GetHeader().Checksum() = CalculateChecksum(*p);
  auto [buf, size] = p->GetBuffer();
  if (size != 32) std::exit(4);
  for (int i = 0; i < 32; ++i) c.image[i] = static_cast<uint8_t>(buf[i]);
  // the exact (unwrapped) sum of the sixteen words, checksum field as zero
  uint32_t exact = 0;
  for (int i = 0; i < 32; i += 2)
    if (i != 28) exact += c.image[i] | c.image[i + 1] << 8;
  if ((exact & 0xFFFF) != c.word_sum) std::exit(5);
  c.word_sum = exact;
}

uint16_t stored(const Case &c) { return static_cast<uint16_t>(c.image[28] | c.image[29] << 8); }

// every byte no helper sets must be 0 (the zeroed heap)
bool unset_bytes_zero(const Case &c) {
  const uint8_t *b = c.image;
  bool ok = !b[8] && !b[9] && !b[10] && !b[11] && !b[24] && !b[30] && !b[31];
  ok = ok && (b[25] & ~(c.rst ? 0x20 : 0x08)) == 0 && (b[25] & (c.rst ? 0x20 : 0x08));
  if (c.rst)
    for (int i : {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 26, 27}) ok = ok && !b[i];
  return ok;
}

Case ack_case(const char *group, uint32_t seq, uint32_t ack, uint16_t wnd, uint32_t sip, uint16_t sport, uint32_t dip,
              uint16_t dport) {
  Case c{false, group, seq, ack, wnd, sip, dip, sport, dport, {}, 0};
  build(c);
  return c;
}

Case rst_case(const char *group, uint32_t ack) {
  Case c{true, group, 0, ack, 0, 0, 0, 0, 0, {}, 0};
  build(c);
  return c;
}

Case random_case(const char *group, bool rst) {
  if (rst) return rst_case(group, next32());
  return ack_case(group, next32(), next32(), static_cast<uint16_t>(next32()), next32(), static_cast<uint16_t>(next32()),
                  next32(), static_cast<uint16_t>(next32()));
}

// a random case whose ack number is then searched until the REF checksum is `want`
Case searched(const char *group, bool rst, uint16_t want) {
  Case c = random_case(group, rst);
  for (uint32_t step = 0; step <= 0x20000; ++step) {
    if (stored(c) == want) return c;
    c.ack += 1 + (step & 1) * 0x10000;  // walks both halves of the number
    build(c);
  }
  std::exit(6);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const uint32_t edge[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0x00FF00FFu, 0xFF00FF00u};
  std::vector<Case> cases;
  // the issue's orientation cases
  cases.push_back(ack_case("example", 5, 7, 9, 1, 2, 0, 0));
  cases.push_back(rst_case("example", 0x01020304u));
  for (uint32_t e : edge) {
    const uint16_t h = static_cast<uint16_t>(e), g = static_cast<uint16_t>(e >> 16);
    cases.push_back(ack_case("edge-seq", e, 1000, 1024, 0x7F000001u, 15500, 0x7F000001u, 15501));
    cases.push_back(ack_case("edge-ack", 1000, e, 1024, 0x7F000001u, 15500, 0x7F000001u, 15501));
    cases.push_back(ack_case("edge-window", 1000, 2000, h, 0x7F000001u, 15500, 0x7F000001u, 15501));
    cases.push_back(ack_case("edge-window", 1000, 2000, g, 0x7F000001u, 15500, 0x7F000001u, 15501));
    cases.push_back(ack_case("edge-source", 1000, 2000, 1024, e, h, 0x7F000001u, 15501));
    cases.push_back(ack_case("edge-destination", 1000, 2000, 1024, 0x7F000001u, 15500, e, g));
    cases.push_back(ack_case("edge-all", e, e, h, e, g, e, h));
    cases.push_back(rst_case("edge-ack", e));
  }
  for (int i = 0; i < 30; ++i) cases.push_back(searched("checksum-0000", i % 3 == 2, 0x0000));
  for (int i = 0; i < 30; ++i) cases.push_back(searched("checksum-ffff", i % 3 == 2, 0xFFFF));
  // the word sum carries out of 16 bits more than once: REF and RFC 1071 differ
  for (int found = 0; found < 30;) {
    Case c = ack_case("carries", next32() | 0xC000C000u, next32() | 0xC000C000u,
                      static_cast<uint16_t>(next32() | 0xC000u), next32() | 0xC000C000u,
                      static_cast<uint16_t>(next32() | 0xC000u), next32() | 0xC000C000u,
                      static_cast<uint16_t>(next32() | 0xC000u));
    if (c.word_sum >> 16 < 2) continue;
    cases.push_back(c);
    ++found;
  }
  for (int i = 0; cases.size() < 250; ++i) cases.push_back(random_case("random", i % 3 == 2));
  // ACK and RST interleaved: a seeded shuffle, so one pass over the fixture is a mixed ring
  for (size_t i = cases.size() - 1; i > 0; --i) std::swap(cases[i], cases[next32() % (i + 1)]);

  std::vector<uint8_t> blob;
  std::string json = "{\n  \"blob\": \"reply_golden.bin\",\n  \"cases\": [";
  int n_rst = 0, n_zero = 0, n_ffff = 0, n_carry = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case &c = cases[i];
    if (!unset_bytes_zero(c)) {
      std::fprintf(stderr, "case %zu: a byte no helper sets is not 0\n", i);
      return 3;
    }
    blob.insert(blob.end(), c.image, c.image + 32);
    n_rst += c.rst, n_zero += stored(c) == 0, n_ffff += stored(c) == 0xFFFF, n_carry += c.word_sum >> 16 >= 2;
    json += std::string(i ? "," : "") + "\n    {\"kind\": \"" + (c.rst ? "rst" : "ack") + "\", \"group\": \"" + c.group +
            "\", \"seq\": " + std::to_string(c.seq) + ", \"ack\": " + std::to_string(c.ack) +
            ", \"wnd\": " + std::to_string(c.wnd) + ", \"src_ip\": " + std::to_string(c.src_ip) +
            ", \"src_port\": " + std::to_string(c.src_port) + ", \"dst_ip\": " + std::to_string(c.dst_ip) +
            ", \"dst_port\": " + std::to_string(c.dst_port) + ", \"ref_checksum\": " + std::to_string(stored(c)) +
            ", \"word_sum\": " + std::to_string(c.word_sum) + "}";
  }
  json += "\n  ],\n  \"blob_bytes\": " + std::to_string(blob.size()) + "\n}\n";
  FILE *f = std::fopen((dir + "/reply_golden.bin").c_str(), "wb");
  if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size()) return 1;
  std::fclose(f);
  f = std::fopen((dir + "/reply_golden.json").c_str(), "w");
  if (!f) return 1;
  std::fputs(json.c_str(), f);
  std::fclose(f);
  std::printf("wrote %zu cases (%d RST, %d with checksum 0x0000, %d with 0xFFFF, %d carrying twice)\n", cases.size(), n_rst,
              n_zero, n_ffff, n_carry);
  return 0;
}
