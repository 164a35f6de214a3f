#!/bin/sh
# Regenerates tests/golden/resend_golden.{bin,json}: queued packets built by the
# reference's own inline helpers and what its resend event
# (SocketInternal::ResendPredicate, include/socket-internal.h:363-390, under
# InternalSendPacketWithResend, include/socket-manager.h:37-51) does to each, on
# a zeroed heap (see gen_resend.cc).
# Build container only: needs /root/reference.  The reference header is
# included where it lies; the binary is written to /tmp, never committed.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
g++ -std=c++17 -O1 -Wall -pthread -I"$REF/include" -o /tmp/tcpck_gen_resend "$HERE/gen_resend.cc"
/tmp/tcpck_gen_resend "$HERE"
