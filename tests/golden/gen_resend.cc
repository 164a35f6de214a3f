// tests/golden/gen_resend.cc -- generates the committed resend fixtures
// (resend_golden.bin + resend_golden.json): queued packets made by the
// REFERENCE's own inline helpers, and what its resend event does to each:
//
//   send:    MakeTcpPacket(n) with payloads of 0, 2, 100, 536 and 1460 bytes under
//            AckHeader (a data segment), and MakeTcpPacket(0) under SynHeader,
//            SynAckHeader and FinHeader (socket-internal.h:17-41); TcpLength and
//            the sequence number through TcpHeader's accessors; SetSource,
//            SetDestination (:52-60), TcpHeaderH2N; SocketManager::SendPacket's
//            two checksum lines (src/socket-manager.cc:9-10), RESTATED here:
//            Checksum() = 0; Checksum() = CalculateChecksum(*p)
//   resend:  the body of SocketInternal::ResendPredicate::operator()
//            (socket-internal.h:376-385) on the reference's own TcpHeader:
//            AcknowledgementNumber() = htonl(rcv_nxt); seq =
//            ntohl(SequenceNumber()); closed -> false; Syn() || Fin() -> snd_una <
//            seq + 1; else snd_una < seq; and for a kept packet the two checksum
//            lines again (InternalSendPacketWithResend -> SendPacket,
//            socket-manager.h:37-51)
//
// The predicate's compare lines are RESTATED in keep_of() below, with the
// citation: SocketInternal itself cannot be linked here (gen_deliver.cc records
// why: it drags in the timer translation unit, which g++ 11 rejects), and the
// predicate reads its control block and state through a live SocketInternal.
// Everything the lines operate on -- the header accessors, Syn(), Fin(), the byte
// order, the checksum -- is the reference's own code.
//
// The heap is zeroed as in gen_reply.cc (TcpPacket's constructor
// default-initialises the header, tcp-header.h:270-273), so the fixture is what
// the reference holds on a fresh heap.
//
// Built and run only in the build container, where /root/reference exists:
//     sh tests/golden/make_resend_golden.sh
// The reference header is #included by path; no reference source is copied.
// Output = data only: per case its inputs and the keep decision (JSON), the whole
// image before the pass and, for a kept image, its 32 header bytes after (blob).
#include "socket-internal.h"

#include <arpa/inet.h>

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

uint64_t rng = 0xA0761D6478BD642Full;  // fixed seed
uint32_t next32() {
  rng ^= rng << 13;
  rng ^= rng >> 7;
  rng ^= rng << 17;
  return static_cast<uint32_t>(rng >> 32);
}

enum Shape { kData, kSyn, kSynAck, kFin };
const char *const kShapeName[] = {"data", "syn", "synack", "fin"};

struct Case {
  const char *group;
  Shape shape;
  uint32_t payload;
  uint32_t seq, snd_una, rcv_nxt;
  bool closed;
  // results
  bool keep, syn, fin;
  std::vector<uint8_t> before;
  uint8_t after[32];
};

void checksum_lines(TcpPacket &p) {  // src/socket-manager.cc:9-10
  p.GetHeader().Checksum() = 0;
  p.GetHeader().Checksum() = CalculateChecksum(p);
}

// socket-internal.h:376-385, on the packet's own header
bool keep_of(TcpPacket &packet, uint32_t snd_una, uint32_t rcv_nxt, bool closed) {
  packet.GetHeader().AcknowledgementNumber() = htonl(rcv_nxt);
  const auto seq = ntohl(packet.GetHeader().SequenceNumber());
  if (closed) {
    return false;
  } else if (packet.GetHeader().Syn() || packet.GetHeader().Fin()) {
    return snd_una < seq + 1;
  } else {
    return snd_una < seq;
  }
}

void run(Case &c) {
  auto p = MakeTcpPacket(c.shape == kData ? c.payload : 0);
  TcpHeader &h = p->GetHeader();
  const uint32_t old_ack = next32();
  const uint16_t wnd = static_cast<uint16_t>(next32());
  switch (c.shape) {
    case kData: AckHeader(c.seq, old_ack, wnd, &h); break;
    case kSyn: SynHeader(c.seq, wnd, &h); break;
    case kSynAck: SynAckHeader(c.seq, old_ack, wnd, &h); break;
    case kFin: FinHeader(c.seq, old_ack, wnd, &h); break;
  }
  if (c.shape == kData) {
    h.TcpLength() = static_cast<uint16_t>(c.payload);
    for (auto it = p->begin(); it != p->end(); ++it) *it = static_cast<char>(next32());
  }
  SetSource(0x0A000001u + (next32() & 0xFF), static_cast<uint16_t>(1024 + (next32() & 0x3FFF)), &h);
  SetDestination(0x0A000101u + (next32() & 0xFF), static_cast<uint16_t>(1024 + (next32() & 0x3FFF)), &h);
  TcpHeaderH2N(h);
  checksum_lines(*p);
  auto [buf, size] = p->GetBuffer();
  c.before.assign(reinterpret_cast<const uint8_t *>(buf), reinterpret_cast<const uint8_t *>(buf) + size);
  if (size != 32 + (c.shape == kData ? c.payload : 0) || CalculateChecksum(*p) != 0) std::exit(4);

  c.syn = h.Syn(), c.fin = h.Fin();
  c.keep = keep_of(*p, c.snd_una, c.rcv_nxt, c.closed);
  if (c.keep) checksum_lines(*p);
  auto [buf2, size2] = p->GetBuffer();
  (void)size2;
  for (int i = 0; i < 32; ++i) c.after[i] = static_cast<uint8_t>(buf2[i]);
  if (c.keep && CalculateChecksum(*p) != 0) std::exit(5);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::vector<Case> cases;
  const uint32_t payloads[] = {0, 2, 100, 536, 1460};
  auto add = [&](const char *group, Shape s, uint32_t payload, uint32_t seq, uint32_t una, bool closed) {
    Case c{group, s, payload, seq, una, next32(), closed, false, false, false, {}, {}};
    run(c);
    cases.push_back(c);
  };
  auto every_shape = [&](const char *group, uint32_t seq, uint32_t una, bool closed, int turn) {
    add(group, kData, payloads[turn % 5], seq, una, closed);
    add(group, kData, payloads[(turn + 2) % 5], seq, una, closed);
    add(group, kSyn, 0, seq, una, closed);
    add(group, kSynAck, 0, seq, una, closed);
    add(group, kFin, 0, seq, una, closed);
  };
  int turn = 0;
  for (uint32_t una : {1000u, 0x80000000u, 0x12345678u, 0xFFFFFFFFu, 0u}) {
    every_shape("seq-equal", una, una, false, turn++);
    every_shape("seq-above-1", una + 1, una, false, turn++);       // (0xFFFFFFFF + 1 wraps to 0)
    every_shape("seq-below-1", una - 1, una, false, turn++);       // (0 - 1 wraps to 0xFFFFFFFF)
    every_shape("seq-far-below", una - 100000, una, false, turn++);
  }
  // snd_una just below 2^32, seq just above 0: the plain compare keeps nothing across the wrap
  for (uint32_t seq : {0u, 1u, 5u, 1460u}) every_shape("wrap", seq, 0xFFFFFFF0u, false, turn++);
  // a SYN and a FIN with seq == 0xFFFFFFFF: seq + 1 is 0
  for (uint32_t una : {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
    add("seq-max", kSyn, 0, 0xFFFFFFFFu, una, false);
    add("seq-max", kSynAck, 0, 0xFFFFFFFFu, una, false);
    add("seq-max", kFin, 0, 0xFFFFFFFFu, una, false);
    add("seq-max", kData, 100, 0xFFFFFFFFu, una, false);
  }
  // a closed socket drops what it would otherwise keep, and what it would drop
  every_shape("closed", 5000, 1000, true, turn++);
  every_shape("closed", 500, 1000, true, turn++);
  while (cases.size() < 210) {
    const uint32_t una = next32();
    const uint32_t seq = una + static_cast<int32_t>(next32() % 6000) - 3000;
    add("random", static_cast<Shape>(next32() % 4), payloads[next32() % 5], seq, una, next32() % 8 == 0);
  }
  // a seeded shuffle, so one pass over the fixture is a mixed queue
  for (size_t i = cases.size() - 1; i > 0; --i) std::swap(cases[i], cases[next32() % (i + 1)]);

  std::vector<uint8_t> blob;
  std::vector<size_t> off;
  for (const Case &c : cases) {
    off.push_back(blob.size());
    blob.insert(blob.end(), c.before.begin(), c.before.end());
  }
  std::string json = "{\n  \"blob\": \"resend_golden.bin\",\n  \"cases\": [";
  int kept = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case &c = cases[i];
    long after_off = -1;
    if (c.keep) {
      after_off = static_cast<long>(blob.size());
      blob.insert(blob.end(), c.after, c.after + 32);
      ++kept;
    }
    json += std::string(i ? "," : "") + "\n    {\"group\": \"" + c.group + "\", \"shape\": \"" + kShapeName[c.shape] +
            "\", \"payload\": " + std::to_string(c.payload) + ", \"seq\": " + std::to_string(c.seq) +
            ", \"snd_una\": " + std::to_string(c.snd_una) + ", \"rcv_nxt\": " + std::to_string(c.rcv_nxt) +
            ", \"closed\": " + (c.closed ? "true" : "false") + ", \"syn\": " + (c.syn ? "true" : "false") +
            ", \"fin\": " + (c.fin ? "true" : "false") + ", \"keep\": " + (c.keep ? "1" : "0") +
            ", \"off\": " + std::to_string(off[i]) + ", \"len\": " + std::to_string(c.before.size()) +
            ", \"after_off\": " + std::to_string(after_off) + "}";
  }
  json += "\n  ],\n  \"blob_bytes\": " + std::to_string(blob.size()) + "\n}\n";
  FILE *f = std::fopen((dir + "/resend_golden.bin").c_str(), "wb");
  if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size()) return 1;
  std::fclose(f);
  f = std::fopen((dir + "/resend_golden.json").c_str(), "w");
  if (!f) return 1;
  std::fputs(json.c_str(), f);
  std::fclose(f);
  std::printf("wrote %zu cases (%d kept), %zu blob bytes\n", cases.size(), kept, blob.size());
  return 0;
}
