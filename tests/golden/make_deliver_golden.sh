#!/bin/sh
# Regenerates tests/golden/deliver_golden.{bin,json}: arrival sequences through
# the reference's own state machine in Estab (src/state.cc:195-223) and the
# payload append of SocketInternal::Accept() (include/socket-internal.h:323-334).
# Build container only: needs /root/reference.  src/state.cc is compiled where
# it lies, as the reference's own state-machine test links it; the binary is
# written to /tmp, never committed.  (The connection's own initial sequence
# number is the reference's random choice, so snd_nxt differs from run to run;
# the fixture records it.)
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
g++ -std=c++17 -O1 -Wall -I"$REF/include" -o /tmp/tcpck_gen_deliver "$HERE/gen_deliver.cc" "$REF/src/state.cc"
/tmp/tcpck_gen_deliver "$HERE" 2>/dev/null
