// tests/golden/gen_deliver.cc -- generates the committed receive-delivery
// fixtures (deliver_golden.bin + deliver_golden.json) by running the
// REFERENCE's own state machine and packet code on arrival sequences:
//
//   connection: two TcpStateManagers (state.h:236-308) and a recording
//            SocketInternalInterface, as test/test-tcp-state-machine.h drives
//            them: the peer's kConnect emits its SYN, whose sequence number is
//            set to a chosen value (so rcv_nxt can sit just below 2^32); the
//            receiver answers SendSynAck and the peer's ACK of it takes the
//            receiver to Estab
//   send:    MakeTcpPacket(len), header fields through TcpHeader's accessors,
//            TcpHeaderH2N, Checksum() = 0; Checksum() = CalculateChecksum(*p)
//            (socket-manager.h:259-260), as gen_receive.cc -- then, for some
//            images, a flipped byte or a wrong checksum
//   receive: MakeNetPacket(wire, n), the verdict CalculateChecksum(*p) == 0,
//            TcpHeaderN2H (ReceivePacket, socket-manager.h:181-184), then
//            RecvPacket's two arms (socket-internal.h:161-171):
//            InvalideCheckSum()(mock) or state_(header)(mock)
//
// The mock records Accept / Discard / SendAck(seq, ack, wnd) / RecvAck.  Its
// Accept() RESTATES the three lines of SocketInternal::Accept()
// (socket-internal.h:325-328: with TcpLength() > 0, insert packet->begin() ..
// packet->end() at the end of recv_buffer_): SocketInternal itself cannot be
// linked here, it drags in the timer translation unit, which g++ 11 rejects.
//
// Built and run only in the build container, where /root/reference exists:
//     sh tests/golden/make_deliver_golden.sh
// The reference headers are #included by path and src/state.cc is compiled
// where it lies; no reference source is copied.  Output = data only: per
// sequence the wire arena, offsets and lengths, the control block before and
// after, per image the verdict and what the mock saw, and the final
// recv_buffer bytes.
#include "state.h"
#include "tcp-header.h"

#include <cstdint>
#include <cstdio>
#include <deque>
#include <memory>
#include <string>
#include <vector>

using namespace tcp_stack;

namespace {

uint64_t rng = 0x9E3779B97F4A7C15ull;  // fixed seed
uint32_t next32() {
  rng ^= rng << 13;
  rng ^= rng >> 7;
  rng ^= rng << 17;
  return static_cast<uint32_t>(rng >> 32);
}

std::string list(const std::vector<uint64_t> &v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "]";
}

class Recorder : public SocketInternalInterface {
 public:
  void SendSyn(uint32_t seq, uint16_t window) override {
    header = TcpHeader();
    header.SetSyn(true);
    header.SequenceNumber() = seq;
    header.Window() = window;
  }
  void SendSynAck(uint32_t seq, uint32_t ack, uint16_t window) override {
    header = TcpHeader();
    header.SetSyn(true);
    header.SetAck(true);
    header.SequenceNumber() = seq;
    header.AcknowledgementNumber() = ack;
    header.Window() = window;
  }
  void SendAck(uint32_t seq, uint32_t ack, uint16_t window) override {
    ++send_ack;
    reply_seq = seq, reply_ack = ack, reply_wnd = window;
  }
  void SendFin(uint32_t, uint32_t, uint16_t) override {}
  void RecvSyn(uint32_t, uint16_t) override {}
  void RecvAck(uint32_t, uint32_t ack_recv, uint16_t) override {
    ++recv_ack;
    peer_ack = ack_recv;
  }
  void RecvFin(uint32_t, uint32_t, uint16_t) override {}
  void Listen() override {}
  void Connected() override { ++connected; }
  // socket-internal.h:323-334, restated (see the header comment)
  void Accept() override {
    ++accept;
    if (current && current->GetHeader().TcpLength() > 0) {
      const size_t before = recv_buffer.size();
      recv_buffer.insert(recv_buffer.end(), current->begin(), current->end());
      appended += recv_buffer.size() - before;
    }
  }
  void Discard() override { ++discard; }
  void SeqOutofRange(uint16_t) override {}
  void SendRst(uint32_t) override {}
  void InvalidOperation() override {}
  void NewConnection() override {}
  void Close() override {}
  void TimeWait() override {}

  void clear() { accept = discard = send_ack = recv_ack = 0, appended = 0, reply_seq = reply_ack = peer_ack = 0, reply_wnd = 0; }

  TcpHeader header;
  std::shared_ptr<TcpPacket> current;
  std::deque<char> recv_buffer;
  int accept = 0, discard = 0, send_ack = 0, recv_ack = 0, connected = 0;
  size_t appended = 0;
  uint32_t reply_seq = 0, reply_ack = 0, peer_ack = 0;
  uint16_t reply_wnd = 0;
};

// what the sender has: consecutive segments, seq advancing by TcpLength
struct Seg {
  size_t payload;
  uint16_t tcp_len;
};
enum Mod { kPlain, kNoAck, kSyn, kAckAhead, kFin };
struct Arrival {
  int seg;
  int damage;  // 0 none; 1 a byte flipped; 2 checksum off by one
  Mod mod;
};

struct Sequence {
  uint32_t peer_seq;  // the sequence number the peer's SYN carries
  std::vector<Seg> segs;
  std::vector<Arrival> arrivals;
};

std::string block(const TcpControlBlock &b) {
  return "{\"rcv_nxt\": " + std::to_string(b.rcv_nxt) + ", \"snd_nxt\": " + std::to_string(b.snd_nxt) +
         ", \"snd_una\": " + std::to_string(b.snd_una) + ", \"rcv_wnd\": " + std::to_string(b.rcv_wnd) +
         ", \"snd_wnd\": " + std::to_string(b.snd_wnd) + "}";
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::vector<Sequence> seqs(2);
  {  // sequence 0: every anomaly once, all the payload sizes
    Sequence &s = seqs[0];
    s.peer_seq = 70000;
    const size_t sizes[] = {100, 0, 536, 1460, 2, 4, 14, 16, 18, 1024, 1448, 2000, 9000, 0, 1460, 536, 100, 1460};
    for (size_t p : sizes) s.segs.push_back({p, static_cast<uint16_t>(p)});
    s.segs.push_back({100, 60});   // 18: TcpLength != payload size (shorter)
    s.segs.push_back({16, 40});    // 19: ... (longer)
    s.segs.push_back({0, 8});      // 20: TcpLength > 0, empty payload
    s.segs.push_back({0, 0});      // 21: pure ACK
    for (size_t p : {1460, 1460, 2, 1448, 1024, 18, 14, 4, 16, 536, 1460, 1460, 1460, 1460, 536, 100, 2, 9000, 2000, 1448,
                     1024, 16, 30, 62})
      s.segs.push_back({p, static_cast<uint16_t>(p)});
    auto &a = s.arrivals;
    for (int k : {0, 1, 2}) a.push_back({k, 0, kPlain});
    a.push_back({2, 0, kPlain});  // a duplicate
    a.push_back({3, 0, kPlain});
    a.push_back({5, 0, kPlain});  // a future segment
    a.push_back({4, 0, kPlain});  // the gap filler
    a.push_back({5, 0, kPlain});  // the future one again
    a.push_back({6, 1, kPlain});  // damaged ...
    a.push_back({7, 0, kPlain});  // ... so these two are ahead of rcv_nxt
    a.push_back({8, 0, kPlain});
    for (int k : {6, 7, 8}) a.push_back({k, 0, kPlain});  // the retransmission and the rest
    a.push_back({9, 0, kNoAck});
    a.push_back({9, 0, kPlain});
    a.push_back({10, 0, kSyn});
    a.push_back({10, 0, kPlain});
    a.push_back({11, 0, kAckAhead});
    a.push_back({11, 0, kPlain});
    a.push_back({12, 2, kPlain});
    a.push_back({12, 0, kPlain});
    for (int k = 13; k <= 22; ++k) a.push_back({k, 0, kPlain});
    a.push_back({21, 0, kPlain});  // the pure ACK again: seq == rcv_nxt no longer
    a.push_back({23, 1, kPlain});
    a.push_back({24, 2, kPlain});
    a.push_back({25, 0, kPlain});
    const int last = static_cast<int>(s.segs.size()) - 1;
    for (int k = 23; k <= last; ++k) a.push_back({k, 0, kPlain});
    a.push_back({last, 0, kPlain});  // the last one twice
  }
  {  // sequence 1: seq wraps 2^32 inside the third segment; ends with a FIN in sequence
    Sequence &s = seqs[1];
    s.peer_seq = 0xFFFFFFFFu - 3000u;
    for (size_t p : {1460, 1448, 536, 0, 2000, 9000, 1024, 100, 18, 16, 14, 4, 2, 1460, 1460, 1460, 536, 1448, 100, 2,
                     64, 66, 126, 130, 1022, 1026, 34, 32, 30})
      s.segs.push_back({p, static_cast<uint16_t>(p)});
    s.segs.push_back({0, 0});  // 29: the FIN
    auto &a = s.arrivals;
    for (int k : {0, 1}) a.push_back({k, 0, kPlain});
    a.push_back({3, 0, kPlain});  // ahead (a pure ACK past segment 2)
    a.push_back({2, 1, kPlain});
    a.push_back({2, 0, kPlain});  // accepted: rcv_nxt wraps
    a.push_back({1, 0, kPlain});  // an old duplicate from before the wrap
    for (int k = 3; k <= 8; ++k) a.push_back({k, 0, kPlain});
    a.push_back({10, 0, kPlain});
    a.push_back({9, 0, kPlain});
    a.push_back({10, 2, kPlain});
    a.push_back({10, 0, kAckAhead});
    for (int k = 10; k <= 14; ++k) a.push_back({k, 0, kPlain});
    a.push_back({15, 0, kSyn});
    a.push_back({15, 1, kPlain});
    a.push_back({16, 0, kPlain});
    a.push_back({17, 0, kPlain});
    for (int k = 15; k <= 28; ++k) a.push_back({k, 0, kPlain});
    a.push_back({29, 0, kFin});  // last image: leaves Estab
  }

  std::vector<uint8_t> blob;
  std::string json = "{\n  \"blob\": \"deliver_golden.bin\",\n  \"sequences\": [";
  int total = 0;
  for (size_t si = 0; si < seqs.size(); ++si) {
    const Sequence &s = seqs[si];
    // the handshake
    TcpStateManager peer, tcp;
    Recorder peer_io, io;
    peer(Event::kConnect, nullptr)(&peer_io);  // SendSyn
    TcpHeader syn = peer_io.header;
    syn.SequenceNumber() = s.peer_seq;
    tcp(syn)(&io);  // Accept, SendSynAck
    if (tcp.GetState() != State::kSynRcvd) return 2;
    TcpHeader ack;
    ack.SetAck(true);
    ack.SequenceNumber() = s.peer_seq + 1;
    ack.AcknowledgementNumber() = io.header.SequenceNumber() + 1;
    ack.Window() = 4096;
    tcp(ack)(&io);  // Accept, Connected
    if (tcp.GetState() != State::kEstab || io.connected != 1) return 2;
    io.clear();
    const TcpControlBlock initial = tcp.GetControlBlock();
    const uint32_t snd_nxt = initial.snd_nxt;

    // the sender's segments: payload bytes and sequence numbers
    std::vector<std::vector<uint8_t>> bytes;
    std::vector<uint32_t> seg_seq;
    uint32_t seq = initial.rcv_nxt;
    for (const Seg &g : s.segs) {
      std::vector<uint8_t> b(g.payload);
      for (auto &c : b) c = static_cast<uint8_t>(next32());
      bytes.push_back(b);
      seg_seq.push_back(seq);
      seq += g.tcp_len;
    }

    // the wire arena: images at even offsets of every value mod 16
    std::vector<uint8_t> wire;
    std::vector<uint64_t> offsets, lengths, damage;
    for (size_t k = 0; k < s.arrivals.size(); ++k) {
      const Arrival &ar = s.arrivals[k];
      const Seg &g = s.segs[ar.seg];
      auto p = MakeTcpPacket(g.payload);
      std::copy(bytes[ar.seg].begin(), bytes[ar.seg].end(), p->begin());
      TcpHeader &h = p->GetHeader();
      h.SourceAddress() = 0x7F000001u;
      h.DestinationAddress() = 0x7F000001u;
      h.PTCL() = 6;
      h.TcpLength() = g.tcp_len;
      h.SourcePort() = 15500;
      h.DestinationPort() = 15501;
      h.SequenceNumber() = seg_seq[ar.seg];
      h.AcknowledgementNumber() = ar.mod == kAckAhead ? snd_nxt + 5 : snd_nxt - (k % 3 == 2 ? 1 : 0);
      h.SetAck(ar.mod != kNoAck);
      h.SetSyn(ar.mod == kSyn);
      h.SetFin(ar.mod == kFin);
      h.SetPsh(k % 4 == 1);
      h.Window() = static_cast<uint16_t>(1024 + 8 * k);
      TcpHeaderH2N(h);
      h.Checksum() = 0;
      h.Checksum() = CalculateChecksum(*p);
      auto [buf, size] = p->GetBuffer();
      std::vector<uint8_t> w(buf, buf + size);
      if (ar.damage == 1) w[(next32() % (size / 2)) * 2 + (k & 1)] ^= static_cast<uint8_t>(1u << (k % 8));
      if (ar.damage == 2) w[28] ^= 1;
      while (wire.size() % 2 || wire.size() % 16 != (2 * k + 6) % 16) wire.push_back(0xA5);
      offsets.push_back(wire.size());
      lengths.push_back(size);
      damage.push_back(ar.damage);
      wire.insert(wire.end(), w.begin(), w.end());
    }
    while (wire.size() % 16) wire.push_back(0xA5);

    // the receive side
    std::vector<uint64_t> ok, accepted, appended, discarded, send_ack, reply_ack, reply_seq, recv_ack;
    long left_at = -1;
    TcpControlBlock final_block = initial;
    for (size_t k = 0; k < offsets.size(); ++k) {
      auto p = MakeNetPacket(reinterpret_cast<const char *>(wire.data() + offsets[k]), lengths[k]);
      const bool good = CalculateChecksum(*p) == 0;
      TcpHeaderN2H(p->GetHeader());
      io.clear();
      if (!good) {
        tcp.InvalideCheckSum()(&io);
      } else {
        io.current = p;
        tcp(p->GetHeader())(&io);
      }
      io.current.reset();
      ok.push_back(good);
      accepted.push_back(io.accept);
      appended.push_back(io.appended);
      discarded.push_back(io.discard);
      send_ack.push_back(io.send_ack);
      reply_ack.push_back(io.reply_ack);
      reply_seq.push_back(io.reply_seq);
      recv_ack.push_back(io.recv_ack);
      if (tcp.GetState() != State::kEstab) {
        if (left_at >= 0 || k + 1 != offsets.size()) return 3;  // only the last image may leave Estab
        left_at = static_cast<long>(k);
      } else {
        final_block = tcp.GetControlBlock();
      }
    }
    std::vector<uint8_t> recv(io.recv_buffer.begin(), io.recv_buffer.end());
    const size_t wire_off = blob.size();
    blob.insert(blob.end(), wire.begin(), wire.end());
    const size_t recv_off = blob.size();
    blob.insert(blob.end(), recv.begin(), recv.end());
    while (blob.size() % 16) blob.push_back(0);
    total += static_cast<int>(offsets.size());

    json += std::string(si ? "," : "") + "\n    {\n      \"wire_off\": " + std::to_string(wire_off) +
            ", \"arena_bytes\": " + std::to_string(wire.size()) + ", \"recv_off\": " + std::to_string(recv_off) +
            ", \"recv_bytes\": " + std::to_string(recv.size()) + ", \"left_estab_at\": " + std::to_string(left_at) +
            ",\n      \"initial\": " + block(initial) + ",\n      \"final\": " + block(final_block) +
            ",\n      \"after_all\": " + block(tcp.GetControlBlock()) + ",\n      \"offsets\": " + list(offsets) +
            ",\n      \"lengths\": " + list(lengths) + ",\n      \"damage\": " + list(damage) + ",\n      \"ok\": " +
            list(ok) + ",\n      \"accepted\": " + list(accepted) + ",\n      \"appended\": " + list(appended) +
            ",\n      \"discarded\": " + list(discarded) + ",\n      \"send_ack\": " + list(send_ack) +
            ",\n      \"reply_ack\": " + list(reply_ack) + ",\n      \"reply_seq\": " + list(reply_seq) +
            ",\n      \"recv_ack\": " + list(recv_ack) + "\n    }";
  }
  json += "\n  ],\n  \"blob_bytes\": " + std::to_string(blob.size()) + "\n}\n";
  FILE *f = std::fopen((dir + "/deliver_golden.bin").c_str(), "wb");
  if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size()) return 1;
  std::fclose(f);
  f = std::fopen((dir + "/deliver_golden.json").c_str(), "w");
  if (!f) return 1;
  std::fputs(json.c_str(), f);
  std::fclose(f);
  std::printf("wrote %zu bytes of deliver fixtures, %d images\n", blob.size(), total);
  return 0;
}
