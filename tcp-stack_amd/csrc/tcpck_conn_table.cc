// tcpck_conn_table.cc -- the connection table's host mirror (include/tcpck.h:
// tcpck_conn_table_set / _erase / _find / _stats) and the rebuild of the image
// tcpck_conn_table_commit uploads (tcpck_demux.hip).
//
// Reference (filixi/TCP-stack): SocketManager::identifier_to_socket_, an
// unordered_map<SocketIdentifier, ...> (include/socket-manager.h:235-245,
// equality include/socket-internal.h:65-69); set is its operator[] / emplace
// (:70-90), erase its erase.  Here: open addressing with linear probing over
// 16-B slots (tcpck_conn_table.h); erase shifts the rest of the run back, so
// the mirror never holds a tombstone either.
//
// Plain host C++ (no HIP).  Not thread-safe, as the header says.
#include "tcpck_conn_table.h"

namespace tcpck {
namespace conn {

namespace {

// The slot of the key, or the empty slot that ends its probe run.
uint32_t locate(const std::vector<Slot> &tab, uint32_t peer_ip, uint32_t ports) {
  const uint32_t mask = static_cast<uint32_t>(tab.size()) - 1;
  uint32_t i = hash(peer_ip, ports) & mask;
  // (entries <= slots / 2: an empty slot is always there)
  while (tab[i].used && !(tab[i].peer_ip == peer_ip && tab[i].ports == ports)) i = (i + 1) & mask;
  return i;
}

}  // namespace

void rebuild(const std::vector<Slot> &mirror, std::vector<Slot> &image, uint32_t &longest_probe, uint64_t &wrapped) {
  image.assign(mirror.size(), Slot{0, 0, 0, 0});
  const uint32_t mask = static_cast<uint32_t>(mirror.size()) - 1;
  longest_probe = 0;
  wrapped = 0;
  for (const Slot &e : mirror) {
    if (!e.used) continue;
    const uint32_t home = hash(e.peer_ip, e.ports) & mask;
    const uint32_t at = locate(image, e.peer_ip, e.ports);
    image[at] = e;
    const uint32_t run = ((at - home) & mask) + 1;  // slots a lookup inspects to find it
    if (run > longest_probe) longest_probe = run;
    if (at < home) ++wrapped;
  }
}

}  // namespace conn
}  // namespace tcpck

using tcpck::conn::Slot;

extern "C" int tcpck_conn_table_set(tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip, uint16_t peer_port,
                                    uint32_t id) {
  if (!t || id == TCPCK_CONN_NONE) return TCPCK_EINVAL;
  const uint32_t ports = tcpck::conn::pack_ports(host_port, peer_port);
  Slot &s = t->mirror[tcpck::conn::locate(t->mirror, peer_ip, ports)];
  if (!s.used) {
    if (t->entries >= t->max_conns) return TCPCK_ENOMEM;
    ++t->entries;
  }
  s = Slot{peer_ip, ports, id, 1};
  return TCPCK_OK;
}

extern "C" int tcpck_conn_table_erase(tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip, uint16_t peer_port) {
  if (!t) return TCPCK_EINVAL;
  std::vector<Slot> &tab = t->mirror;
  const uint32_t mask = t->slots - 1;
  uint32_t hole = tcpck::conn::locate(tab, peer_ip, tcpck::conn::pack_ports(host_port, peer_port));
  if (!tab[hole].used) return TCPCK_OK;
  // close the hole: every later entry of the run whose home slot does not lie
  // in (hole, its slot] moves back into it
  for (uint32_t j = (hole + 1) & mask; tab[j].used; j = (j + 1) & mask) {
    const uint32_t home = tcpck::conn::hash(tab[j].peer_ip, tab[j].ports) & mask;
    if (((j - home) & mask) >= ((j - hole) & mask)) {
      tab[hole] = tab[j];
      hole = j;
    }
  }
  tab[hole] = Slot{0, 0, 0, 0};
  --t->entries;
  return TCPCK_OK;
}

extern "C" int tcpck_conn_table_find(const tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip,
                                     uint16_t peer_port, uint32_t *id) {
  if (!t || !id) return TCPCK_EINVAL;
  const Slot &s = t->mirror[tcpck::conn::locate(t->mirror, peer_ip, tcpck::conn::pack_ports(host_port, peer_port))];
  *id = s.used ? s.id : TCPCK_CONN_NONE;
  return TCPCK_OK;
}

extern "C" int tcpck_conn_table_stats(const tcpck_conn_table *t, uint64_t *slots, uint64_t *entries,
                                      uint32_t *longest_probe, uint64_t *wrapped) {
  if (!t) return TCPCK_EINVAL;
  if (slots) *slots = t->committed ? t->slots : 0;
  if (entries) *entries = t->image_entries;
  if (longest_probe) *longest_probe = t->image_longest;
  if (wrapped) *wrapped = t->image_wrapped;
  return TCPCK_OK;
}
