#!/bin/sh
# Regenerates tests/golden/reply_golden.{bin,json}: the ACK and RST datagrams of
# SocketInternal::SendAck (include/socket-internal.h:293-299) and of
# ReceivePacket's no-socket branch (include/socket-manager.h:201-207), built by
# the reference's own inline helpers on a zeroed heap (see gen_reply.cc).
# Build container only: needs /root/reference.  The reference header is
# included where it lies; the binary is written to /tmp, never committed.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
g++ -std=c++17 -O1 -Wall -pthread -I"$REF/include" -o /tmp/tcpck_gen_reply "$HERE/gen_reply.cc"
/tmp/tcpck_gen_reply "$HERE"
