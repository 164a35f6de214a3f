// tcpck_conn_table.h -- the connection table shared by its host mirror
// (tcpck_conn_table.cc, plain C++) and its device side (tcpck_demux.hip: the
// image's allocation and upload, the demux kernel).  Not installed.
//
// One slot is 16 B -- key, id and an occupied marker -- so a probe step is one
// 16-B load.  The key is ReceivePacket's (include/socket-manager.h:187-196)
// packed as the host-order header holds it: peer_ip is the u32 at header byte
// 0, `ports` the u32 at header byte 12 (source = peer port in the low half,
// destination = host port in the high half); a listener's key is (0, host_port
// << 16).  Linear probing from hash(key) & (slots - 1); slots is a power of two
// >= 2 * max_conns, so an empty slot always ends a probe.
#pragma once

#include <cstdint>
#include <vector>

#include "tcpck.h"

#if defined(__HIPCC__)
#define TCPCK_HD __host__ __device__ inline
#else
#define TCPCK_HD inline
#endif

namespace tcpck {
namespace conn {

struct Slot {
  uint32_t peer_ip;
  uint32_t ports;  // peer_port | host_port << 16
  uint32_t id;
  uint32_t used;   // 0: empty (the whole slot is 0), 1: occupied
};
static_assert(sizeof(Slot) == 16, "one 16-B load per probe step");

constexpr uint32_t kMaxConns = 1u << 22;
constexpr uint32_t kMinSlots = 64;

TCPCK_HD uint32_t pack_ports(uint16_t host_port, uint16_t peer_port) {
  return static_cast<uint32_t>(peer_port) | static_cast<uint32_t>(host_port) << 16;
}

// Consecutive ports and consecutive addresses (what real tables hold) must not
// land in consecutive slots: two multiplies and two xor-shifts spread both.
TCPCK_HD uint32_t hash(uint32_t peer_ip, uint32_t ports) {
  uint32_t h = peer_ip * 0x9E3779B1u ^ ports * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 13;
  return h;
}

// The image of `entries` (the occupied slots of any table of the same slot
// count, in slot order) rebuilt into `image` (zeroed here); longest probe run
// and wrapped entries as tcpck_conn_table_stats reports them.
void rebuild(const std::vector<Slot> &mirror, std::vector<Slot> &image, uint32_t &longest_probe, uint64_t &wrapped);

}  // namespace conn
}  // namespace tcpck

struct tcpck_conn_table {
  int device = -1;  // -1: host only (created without a context)
  uint32_t max_conns = 0;
  uint32_t slots = 0;  // power of two, <= 2^23
  uint64_t entries = 0;                  // of the mirror
  std::vector<tcpck::conn::Slot> mirror;  // the live table: set / erase / find
  std::vector<tcpck::conn::Slot> image;   // as last committed (host copy of the device image)
  tcpck::conn::Slot *d_image = nullptr;   // slots * 16 B on `device`
  bool committed = false;
  uint64_t image_entries = 0, image_wrapped = 0;
  uint32_t image_longest = 0;
};
