/*
 * tcpck.h -- C-ABI of the MI355X (gfx950) TCP checksum library, libtcpck.so.
 *
 * Drop-in boundary for the one per-byte hot path of filixi/TCP-stack:
 *
 *   friend uint16_t CalculateChecksum(const TcpPacket &)   include/tcp-header.h:252-263
 *
 * and its three call sites:
 *
 *   send, insert   src/socket-manager.cc:9-10, include/socket-manager.h:259-260
 *                  (zero TcpHeader::Checksum(), compute, store raw)
 *   receive,verify include/socket-manager.h:182   (CalculateChecksum(pkt) == 0)
 *
 * Plain pointers and sizes only.  Every entry point returns an int status
 * (TCPCK_OK = 0, negative on error) and never throws.  The reference has no
 * error path (odd sizes are an out-of-bounds read, tcp-header.h:259-260); here
 * odd lengths are rejected with TCPCK_EINVAL where the host can see them, and
 * documented as a precondition for device-resident descriptor arrays.
 *
 * Arithmetic (mode TCPCK_MODE_REF, the default and the parity mode):
 *     checksum = ~(sum of little-endian u16 words of the image mod 2^16) & 0xFFFF
 * i.e. the reference's u32 accumulation with no end-around-carry fold.  The
 * opt-in TCPCK_MODE_RFC1071 folds carries (one's complement, RFC 1071); it is
 * NOT what the reference computes.
 *
 * An "image" is the 32-byte TcpHeader (12-byte pseudo-header + 20-byte TCP
 * header, tcp-header.h:188-190) followed by the payload, contiguous, exactly the
 * bytes of TcpPacket::GetBuffer() (tcp-header.h:265-267).  The checksum field is
 * bytes 28-29 (TcpHeader::Checksum(), tcp-header.h:177), stored raw (host order,
 * no htons), as the reference does.
 */
#ifndef TCPCK_H_
#define TCPCK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCPCK_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
#define TCPCK_OK 0
#define TCPCK_EINVAL (-22)   /* bad argument: odd length/offset, null, overflow */
#define TCPCK_ENOMEM (-12)   /* host or device allocation failed               */
#define TCPCK_ENODEV (-19)   /* no such HIP device                             */
#define TCPCK_EHIP (-1000)   /* HIP runtime error e: returned as TCPCK_EHIP - e */

/* ---- arithmetic modes --------------------------------------------------- */
#define TCPCK_MODE_REF 0     /* bit-exact to tcp-header.h:252-263 (mod 2^16)   */
#define TCPCK_MODE_RFC1071 1 /* opt-in one's complement, end-around carry      */

/* ---- batch operations --------------------------------------------------- */
#define TCPCK_OP_CHECKSUM 0  /* out[k] (u16) = checksum of image k              */
#define TCPCK_OP_FILL 1      /* zero bytes 28-29 of image k, compute, store the
                                result there in place (send path); out[k] (u16)
                                also receives it unless out == NULL.  len >= 30.
                                Only bytes 28-29 change; for packed images of
                                <= 128 B the kernel may store the image's other
                                16-B chunks back unchanged (never bytes outside
                                an image)                                       */
#define TCPCK_OP_VERIFY 2    /* out[k] (u8) = (checksum of image k == 0)
                                (receive path, socket-manager.h:182)            */
#define TCPCK_OP_RECEIVE 3   /* ReceivePacket's front half (socket-manager.h:
                                182-184): out[k] (u8) as VERIFY, on the network-
                                order image; then image k's 32-B header is
                                converted to host order in place (TcpHeaderN2H,
                                see tcpck_batch_header_swap).  Images >= 32 B.
                                The VERIFY pass, then the header pass, on the
                                stream.  Device batches only (not
                                tcpck_host_batch_*).  tcpck_batch_receive can
                                write the headers to a dense array instead. */

/* ---- layout hints (tcpck_layout.flags) ---------------------------------- */
#define TCPCK_LAYOUT_PACKED 1u /* images are back to back in index order:
                                  offsets[k+1] == offsets[k] + lengths[k]      */
#define TCPCK_LAYOUT_SORTED 2u /* images in index order, apart: offsets[k+1] >=
                                  offsets[k] + lengths[k] (receive slots, rings);
                                  a wrong SORTED hint costs speed, never
                                  correctness                                  */

/* Optional description of a variable-length batch.  Zero fields = unknown.
 * Used only to choose a kernel; a wrong hint never changes results, except
 * that TCPCK_LAYOUT_PACKED must be true when set. */
typedef struct tcpck_layout {
  uint64_t total_bytes; /* sum of lengths                                     */
  uint32_t min_len;     /* smallest image length                              */
  uint32_t max_len;     /* largest image length                               */
  uint32_t flags;       /* TCPCK_LAYOUT_*                                     */
  uint32_t reserved;
} tcpck_layout;

typedef struct tcpck_ctx tcpck_ctx;
typedef void *tcpck_stream; /* a hipStream_t; NULL = the device's null stream */

/* ---- library ------------------------------------------------------------ */
int tcpck_abi_version(void);
const char *tcpck_strerror(int status);
/* 1 when the library's gfx950 code object can run on `device`, else 0. */
int tcpck_device_supported(int device);

/* ---- context: one per device; owns no hidden global HIP state ------------
 * A FILL without a results buffer (the reference's call shape,
 * socket-manager.cc:9-10 stores into the packet only) whose AUTO form reads
 * the results back writes them to one of the context's 4 results-scratch
 * slots of 16 MiB (8M images per launch chunk), allocated on the first such
 * call, so it runs the same two-pass forms as a FILL with a buffer.  FILLs
 * on different streams take different slots and overlap; a slot's reuse waits
 * (on the caller's stream, asynchronously) for its previous user's work.  On a
 * stream under capture (HIP graphs), or when the slots cannot be allocated,
 * such a FILL runs AUTO's in-stream form instead (same bytes, no slot, no
 * event); a refused allocation is tried again 64 out-less FILLs later.
 * Context creation allocates nothing on the device. */
int tcpck_ctx_create(int device, tcpck_ctx **out);
int tcpck_ctx_destroy(tcpck_ctx *ctx);
int tcpck_ctx_device(const tcpck_ctx *ctx);

/* ---- single image, host memory (the per-packet drop-in) ------------------
 * Replaces CalculateChecksum(const TcpPacket&) (tcp-header.h:252-263) for one
 * packet at a time: one image is far below a kernel launch in cost, so it is
 * computed on the calling thread.  Reentrant, no allocation. */
int tcpck_checksum16(const void *image, size_t len, int mode, uint16_t *out);
/* Send-side insertion on one host image (socket-manager.cc:9-10). */
int tcpck_fill16(void *image, size_t len, int mode, uint16_t *out);
/* Incremental update of a stored checksum when one aligned u16 word of the
 * image changes from old_word to new_word (retransmit ACK rewrite,
 * socket-internal.h:376-377), exact in the selected mode. */
uint16_t tcpck_update16(uint16_t checksum, uint16_t old_word, uint16_t new_word, int mode);

/* ---- batched, device-resident: the hot path ------------------------------
 * Fixed stride: image k is d_arena[k*stride, k*stride + len).
 * d_arena even (the u16 words of an image sit at even addresses, as in any
 * malloc'd TcpPacket buffer); stride and len even (stride >= len); count images.
 * d_out: u16[count] (CHECKSUM/FILL) or u8[count] (VERIFY); FILL takes NULL
 * (the results then go to the context's scratch, see tcpck_ctx_create).
 * Asynchronous on `stream`; nothing is allocated; no host synchronisation. */
int tcpck_batch_fixed(tcpck_ctx *ctx, int op, int mode, void *d_arena,
                      uint64_t stride, uint32_t len, uint64_t count, void *d_out,
                      tcpck_stream stream);

/* Variable length: image k is d_arena[d_offsets[k], d_offsets[k] + d_lengths[k]).
 * d_arena even; offsets and lengths must be even (precondition: the device
 * arrays are not read by the host).  `layout` may be NULL. */
int tcpck_batch_var(tcpck_ctx *ctx, int op, int mode, void *d_arena,
                    const uint64_t *d_offsets, const uint32_t *d_lengths,
                    uint64_t count, void *d_out, const tcpck_layout *layout,
                    tcpck_stream stream);

/* ---- batched retransmit: ACK rewrite, incremental checksum update --------
 * The resend path: ResendPredicate rewrites the ACK number of each queued
 * packet (include/socket-internal.h:376-377, AcknowledgementNumber() =
 * htonl(rcv_nxt)) and SendPacket then recomputes the whole checksum
 * (src/socket-manager.cc:9-10).  Here, for every image k: bytes 20-23
 * (TCPCK_ACK_OFFSET, AcknowledgementNumber) := htonl(ack_k), and the stored
 * checksum (bytes 28-29) is updated from the two old and new u16 words --
 * C' = ~(~C - old + new) mod 2^16 (TCPCK_MODE_REF) or RFC 1624 eqn. 3
 * (TCPCK_MODE_RFC1071) -- which equals the full recompute whenever C was the
 * valid checksum of the old image (e.g. written by TCPCK_OP_FILL).
 * d_offsets == NULL: image k at k * stride (stride even, >= 30); else image k
 * at d_offsets[k] (precondition: even, image >= 30 B).  d_acks: u32[count],
 * host order; NULL: every image gets `ack`.  d_out: u16[count] receiving C'
 * (may be NULL).  Asynchronous on `stream`. */
#define TCPCK_ACK_OFFSET 20
int tcpck_batch_set_ack(tcpck_ctx *ctx, int mode, void *d_arena, const uint64_t *d_offsets,
                        uint64_t stride, uint64_t count, const uint32_t *d_acks, uint32_t ack,
                        uint16_t *d_out, tcpck_stream stream);

/* ---- batched resend pass: ResendPredicate over a whole send queue ---------
 * The reference's resend event, per queued packet:
 * SocketManager::InternalSendPacketWithResend (include/socket-manager.h:37-51)
 * calls SocketInternal::ResendPredicate::operator()
 * (include/socket-internal.h:363-390), which rewrites the ACK number to
 * htonl(rcv_nxt) (:376-377), decides from snd_una, the packet's sequence number
 * and its SYN / FIN bits whether the packet is still owed (:378-385; a dead
 * socket, :371-373, or a closed one, :379-380, drops it), and then either sends
 * the packet again through SendPacket (src/socket-manager.cc:6-12: the checksum
 * recomputed) and re-queues it, or drops it from the queue.  Here, for a queue
 * of many connections in one call: a predicate per image, tcpck_batch_set_ack's
 * 6-byte patch on the survivors, and a stable compaction of the queue's
 * descriptor arrays.  The dense (offsets, lengths) list of the survivors is the
 * retransmit ring -- already what tcpck_batch_var / tcpck_batch_receive take,
 * TCPCK_LAYOUT_SORTED preserved because the compaction is stable -- and the
 * queue of the next pass.
 *
 * Image k: at k * stride, `len` bytes (d_offsets == NULL), else at d_offsets[k],
 * d_lengths[k] bytes.  Its connection: c = d_conn ? d_conn[k] : 0.  d_snd: one
 * tcpck_snd_state per connection, n_conns of them, refreshed by the caller.
 *   dropped untouched (keep = 0, not one byte of the image written): an odd
 *     offset or length; a length below 32; a range that does not fit in
 *     [0, arena_bytes); c >= n_conns -- the dead weak_ptr of :371-373,
 *     TCPCK_CONN_NONE lands here, and no state block outside [0, n_conns) is
 *     read, whatever the arrays hold; d_snd[c].flags & TCPCK_SND_CLOSED
 *     (:379-380).  The reference rewrites the ACK number before it looks at the
 *     closed state and then destroys the packet: that rewrite is unobservable,
 *     so here the image stays as it was.
 *   read from the header: seq = the big-endian u32 at bytes 16-19
 *     (ntohl(SequenceNumber())); byte 25's SYN 0x40 and FIN 0x80.
 *   TCPCK_RESEND_REF (:381-385): keep iff snd_una < seq + 1 for a SYN or FIN
 *     image (u32: 0xFFFFFFFF + 1 is 0), iff snd_una < seq otherwise.  Plain
 *     unsigned compares, as the reference, with its consequences kept: a data
 *     image whose seq == snd_una is dropped (wholly unacknowledged as it is), and
 *     nothing is kept across a wrap of snd_una (snd_una just below 2^32, seq
 *     just above 0: dropped).
 *   TCPCK_RESEND_SERIAL (opt-in, like TCPCK_MODE_RFC1071; NOT what the
 *     reference computes): n = TcpLength (the big-endian u16 at bytes 10-11) + 1
 *     for a SYN or FIN image; keep iff n > 0 and (int32_t)(seq + n - snd_una) >
 *     0 -- RFC 793 serial arithmetic: some sequence number of the image is not
 *     yet acknowledged.
 *   kept: bytes 20-23 := htonl(d_snd[c].rcv_nxt) and bytes 28-29 updated from
 *     the old and new words exactly as tcpck_batch_set_ack does in `mode` -- the
 *     reference's full recompute whenever the stored checksum was valid.  No
 *     other byte of the arena changes.  The call equals tcpck_batch_set_ack on
 *     exactly the kept images, each image's ack its connection's rcv_nxt.
 * Outputs, each of the five arrays may be NULL: d_keep[k] = 0 or 1; the
 * survivors dense and in queue order: d_out_offsets[j], d_out_lengths[j],
 * d_out_conn[j] (0 when d_conn is NULL), d_src[j] = k; *d_count (device, u64) =
 * the number kept.  When that exceeds out_cap only the first out_cap entries of
 * each list are written, *d_count still holds the total and every kept image is
 * still patched; the patch is idempotent under the same d_snd, so a caller that
 * ran short runs again with longer lists.  Nothing is written past any list's
 * min(total, out_cap) entries or past d_keep[count).  Preconditions: the images
 * of a queue are disjoint; the output lists overlap neither the input lists nor
 * each other (to iterate, ping-pong two sets of lists).  d_scratch: device
 * memory of the size tcpck_resend_scratch_bytes(count, &bytes) gives (never 0),
 * its contents undefined before and after.  Asynchronous on `stream`; nothing is
 * allocated; no host synchronisation; the same inputs give the same bytes.
 * count == 0 is TCPCK_OK and sets *d_count = 0 in stream order when d_count is
 * not NULL.  TCPCK_EINVAL, nothing launched or written: ctx NULL; a bad mode or
 * rule; count > 2^31; with count > 0 a NULL d_arena, d_snd (when n_conns > 0),
 * d_count or d_scratch; d_offsets and d_lengths not both NULL or both set; the
 * fixed form with an odd stride or len, len < 32 or stride < len; a misaligned
 * pointer (d_arena 2-B; the u32 arrays 4-B; the u64 arrays and d_count 8-B;
 * d_snd and d_scratch 16-B).  tcpck_resend_scratch_bytes: TCPCK_EINVAL for
 * bytes NULL or count > 2^31. */
typedef struct tcpck_snd_state {      /* 16 B per connection: what ResendPredicate reads */
  uint32_t snd_una, rcv_nxt, flags, reserved;
} tcpck_snd_state;
#define TCPCK_SND_CLOSED 1u           /* state_.GetState() == State::kClosed */
#define TCPCK_RESEND_REF 0            /* the reference's compare, bit for bit */
#define TCPCK_RESEND_SERIAL 1         /* opt-in: RFC 793 serial arithmetic */
int tcpck_resend_scratch_bytes(uint64_t count, size_t *bytes);
int tcpck_batch_resend(tcpck_ctx *ctx, int mode, int rule, void *d_arena, uint64_t arena_bytes,
                       uint64_t stride, uint32_t len, const uint64_t *d_offsets, const uint32_t *d_lengths,
                       const uint32_t *d_conn, const tcpck_snd_state *d_snd, uint32_t n_conns, uint64_t count,
                       uint8_t *d_keep, uint64_t *d_out_offsets, uint32_t *d_out_lengths, uint32_t *d_out_conn,
                       uint32_t *d_src, uint64_t out_cap, uint64_t *d_count, void *d_scratch, tcpck_stream stream);
/* The same contract on host memory: plain host C++, reentrant, no device, no
 * scratch; the number kept is returned through n_kept.  The CPU fallback and the
 * second implementation the device call is tested against.  It checks the same
 * clauses (n_kept in d_count's place); every case a host could see in the
 * arrays' contents is, by the rule above, a dropped image and not an error.
 * Nothing is written on an error. */
int tcpck_resend_images(int mode, int rule, void *h_arena, uint64_t arena_bytes, uint64_t stride, uint32_t len,
                        const uint64_t *h_offsets, const uint32_t *h_lengths, const uint32_t *h_conn,
                        const tcpck_snd_state *h_snd, uint32_t n_conns, uint64_t count, uint8_t *h_keep,
                        uint64_t *h_out_offsets, uint32_t *h_out_lengths, uint32_t *h_out_conn, uint32_t *h_src,
                        uint64_t out_cap, uint64_t *n_kept);

/* ---- batched header byte order: TcpHeaderN2H / TcpHeaderH2N -------------
 * ReceivePacket verifies the network-order image and then converts its header
 * to host order (include/socket-manager.h:182-184); TcpHeaderN2H and
 * TcpHeaderH2N (include/tcp-header.h:193-221) are the same permutation: u32
 * byte swaps of bytes 0-3, 4-7, 16-19, 20-23 (addresses, seq, ack) and u16
 * swaps of 10-11, 12-13, 14-15, 26-27, 30-31 (TcpLength, ports, window,
 * urgent pointer); bytes 8-9, 24-25, 28-29 and the payload are untouched.
 * Applied in place to the first 32 bytes of every image: image k at
 * k * stride (d_offsets == NULL; stride even, >= 32) or at d_offsets[k]
 * (precondition: even, image >= 32 B).  d_arena even.  A receive batch is
 * tcpck_batch_*(TCPCK_OP_VERIFY) then this call on the same stream.
 * Asynchronous on `stream`. */
#define TCPCK_HEADER_BYTES 32
int tcpck_batch_header_swap(tcpck_ctx *ctx, void *d_arena, const uint64_t *d_offsets,
                            uint64_t stride, uint64_t count, tcpck_stream stream);

/* ---- batched receive: verdicts + host-order headers -----------------------
 * ReceivePacket's front half (include/socket-manager.h:181-185) for a batch:
 * d_ok[k] (u8) = (CalculateChecksum(image k) == 0) on the network-order
 * image, and image k's header in host order (TcpHeaderN2H).  Layout: image k
 * at k * stride, `len` bytes (d_offsets == NULL; len >= 32, even) or at
 * d_offsets[k], d_lengths[k] bytes (precondition: >= 32; `layout` as in
 * tcpck_batch_var, may be NULL).  d_arena even.
 *   d_hdr == NULL: headers converted in place (== TCPCK_OP_RECEIVE);
 *   d_hdr != NULL: 4-B aligned, 32 * count bytes: header k in host order at
 *                  d_hdr + 32 k, the arena left as received.  One dense array
 *                  of whole lines instead of one partial-line write per image
 *                  (the cheaper form on this part, profiles/DESIGN_history_r01-r04.md "Receive path").
 * Asynchronous on `stream`. */
int tcpck_batch_receive(tcpck_ctx *ctx, int mode, void *d_arena, uint64_t stride, uint32_t len,
                        const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count,
                        uint8_t *d_ok, void *d_hdr, const tcpck_layout *layout, tcpck_stream stream);

/* ---- batched receive delivery: accepted payloads -> the receive stream ----
 * The receive side's per-byte loop: SocketInternal::Accept() appends an
 * accepted packet's payload (packet->begin()..end()) to recv_buffer_, byte by
 * byte through a deque (include/socket-internal.h:323-334).  Here, for a batch:
 * image k is laid out as in tcpck_batch_receive (at k * stride, `len` bytes, or
 * at d_offsets[k], d_lengths[k] bytes; lengths even, >= 32), and for every k
 * with d_dst[k] != TCPCK_DELIVER_SKIP
 *     d_recv[d_dst[k], d_dst[k] + len_k - 32) := image bytes [32, len_k).
 * Every other byte of d_recv keeps its value.  An image whose d_dst[k] is odd,
 * or whose range does not fit in recv_bytes (or whose length or offset is odd,
 * or whose length is below 32 or above 16 MiB), is skipped whole: no partial write
 * and no write outside [0, recv_bytes) happens, whatever the device arrays
 * hold.  The arena is only read.  Preconditions: the destination ranges of
 * different images are disjoint (with overlap, which image's bytes land is
 * unspecified); d_recv does not overlap the arena.  d_arena even; d_recv 16-B
 * aligned; d_dst: u64[count].  d_dst comes from tcpck_plan_deliver (below) or
 * any other source.  Asynchronous on `stream`; nothing is allocated; no host
 * synchronisation. */
#define TCPCK_DELIVER_SKIP UINT64_MAX
int tcpck_batch_deliver(tcpck_ctx *ctx, const void *d_arena, uint64_t stride, uint32_t len,
                        const uint64_t *d_offsets, const uint32_t *d_lengths, uint64_t count,
                        const uint64_t *d_dst, void *d_recv, uint64_t recv_bytes, tcpck_stream stream);

/* The host planner: which images of an arrival sequence the connection accepts
 * and where their payloads go.  Plain host code, reentrant, no device.  It
 * walks the images in arrival order as SocketInternal::RecvPacket
 * (include/socket-internal.h:161-171) followed by Estab::operator()(const
 * TcpHeader &, ...) (src/state.cc:195-223) does.  h_hdr: 32 * count bytes of
 * host-order headers as tcpck_batch_receive writes them with d_hdr != NULL
 * (TcpLength u16 at byte 10, seq u32 at 16, ack u32 at 20, flags at byte 25 --
 * the reference's bits: ACK 0x08, SYN 0x40, FIN 0x80 -- window u16 at 26);
 * h_ok: the verdicts; h_lengths: the image lengths (NULL: every image `len`);
 * odd lengths or lengths < 32 return TCPCK_EINVAL.  Per image k:
 *   !h_ok[k]      verdict BAD_SUM | SEND_ACK, h_ack[k] = rcv_nxt, no state
 *                 change (TcpStateManager::InvalideCheckSum);
 *   accepted      IsAck (ACK set, SYN and FIN clear), ack <= snd_nxt (a plain
 *                 unsigned compare, as the reference) and seq == rcv_nxt:
 *                 snd_una = max(ack, snd_una), rcv_nxt = seq + TcpLength (u32
 *                 wrap), rcv_wnd = window; ACCEPT, and SEND_ACK iff TcpLength >
 *                 0; h_ack[k] = the new rcv_nxt.  The payload is appended iff
 *                 TcpLength > 0 and len_k > 32: PAYLOAD, h_dst[k] =
 *                 st->delivered, delivered += len_k - 32 -- the reference
 *                 appends begin()..end(), len_k - 32 bytes, whatever TcpLength
 *                 says;
 *   anything else verdict 0, h_dst[k] = TCPCK_DELIVER_SKIP, h_ack[k] = rcv_nxt.
 * The walk stops with *consumed = k before an image that would leave Estab
 * (its FIN branch: IsFin, ack <= snd_nxt, seq == rcv_nxt) and before a payload
 * that does not fit in recv_bytes; images from k on get SKIP, verdict 0 and
 * h_ack = rcv_nxt, and *st holds the state reached.  Otherwise *consumed =
 * count.  h_dst[k] is TCPCK_DELIVER_SKIP wherever PAYLOAD is not set.
 * TCPCK_EINVAL: st or consumed NULL; with count > 0 any other pointer but
 * h_lengths NULL; a bad length (above); st->delivered > recv_bytes.  Nothing
 * is written on an error. */
typedef struct tcpck_rcv_state { /* the TcpControlBlock fields Estab reads and writes */
  uint32_t rcv_nxt, snd_nxt, snd_una;
  uint16_t rcv_wnd, reserved;
  uint64_t delivered;            /* bytes appended to the receive stream so far; between calls the
                                    caller may lower it (to an even value) once it has consumed the
                                    window's front: the next payload lands at the new value */
} tcpck_rcv_state;
#define TCPCK_RCV_ACCEPT 1u   /* Estab's data/ACK branch took the image            */
#define TCPCK_RCV_PAYLOAD 2u  /* ... and Accept() appends its payload (h_dst[k] set) */
#define TCPCK_RCV_SEND_ACK 4u /* the reference replies SendAck(snd_nxt, h_ack[k], .) */
#define TCPCK_RCV_BAD_SUM 8u  /* !ok: InvalideCheckSum(), Discard + SendAck           */
int tcpck_plan_deliver(const void *h_hdr, const uint8_t *h_ok, const uint32_t *h_lengths, uint32_t len,
                       uint64_t count, tcpck_rcv_state *st, uint64_t recv_bytes,
                       uint64_t *h_dst, uint8_t *h_verdict, uint32_t *h_ack, uint64_t *consumed);

/* ---- receive demultiplex: which connection an image belongs to -------------
 * A receive ring holds datagrams of many connections.  The reference, per
 * packet, between TcpHeaderN2H and RecvPacket: SocketManager::ReceivePacket
 * (include/socket-manager.h:181-208) finds the socket in identifier_to_socket_
 * (FindInternal, :235-245), an unordered_map find under the manager's mutex:
 *   key       host_port = DestinationPort(), peer_ip = SourceAddress(),
 *             peer_port = SourcePort(); the host address is the manager's own
 *             ip_ -- the packet's DestinationAddress() is NOT looked at, so a
 *             datagram addressed elsewhere still finds the socket (:187-196);
 *   listener  Syn() && !Ack() looks up (host_port, 0, 0); everything else --
 *             SYN+ACK and a packet with neither flag included -- the full key;
 *   equality  exact on all fields (include/socket-internal.h:65-69);
 *   checksum  the lookup does not depend on the verdict; a found socket gets
 *             RecvPacket(packet, ok); not found and ok: a RST whose sequence
 *             number is the packet's acknowledgement number (RstHeader,
 *             socket-internal.h:43-50); not found and !ok: nothing.
 *
 * The connection table: the map's keys with a caller-chosen u32 id each, a
 * host mirror (set / erase / find) and a device image (commit) the demux kernel
 * probes.  Open addressing, linear probing, 16-B slots, a power-of-two slot
 * count >= 2 * max_conns (at least 64), so an empty slot always ends a probe;
 * the image is rebuilt from the entries at every commit (no tombstones).  The
 * reference's hash is not observable; the one here is the library's own.
 * Listeners are ordinary entries with peer_ip = 0, peer_port = 0.
 *   create   max_conns in [1, 2^22].  ctx != NULL: the image's device memory is
 *            allocated here, once, on the context's device (the context must
 *            outlive the table's last use).  ctx == NULL: a host-only table --
 *            set / erase / find / commit / stats work (commit rebuilds the host
 *            image and uploads nothing), tcpck_batch_demux refuses it.
 *   set      adds the key or overwrites its id (identifier_to_socket_[key] =
 *            ..., socket-manager.h:70-90).  id == TCPCK_CONN_NONE:
 *            TCPCK_EINVAL.  A new key beyond max_conns: TCPCK_ENOMEM, the
 *            table as it was.
 *   erase    an absent key is TCPCK_OK (unordered_map::erase).
 *   find     reads the host mirror (committed or not): *id = the key's id or
 *            TCPCK_CONN_NONE.
 *   commit   rebuilds the image from the mirror's entries and uploads it on
 *            `stream`.  Control plane: it blocks until the upload is done.
 *            Demux launches enqueued on that stream after it returns see
 *            exactly the committed entries, launches enqueued there earlier
 *            the previous commit; ordering against other streams is the
 *            caller's.
 *   stats    of the image as last committed (all 0 before the first commit):
 *            *slots, *entries, *longest_probe = the most slots a lookup
 *            inspects to find an entry, *wrapped = the entries whose probe run
 *            passes the end of the slot array.  Any out-pointer may be NULL.
 * TCPCK_EINVAL: a NULL table or (create, find) out-pointer, max_conns out of
 * range.  Not thread-safe: calls on one table are the caller's to serialise
 * (the reference runs them under the manager's mutex). */
#define TCPCK_CONN_NONE UINT32_MAX
typedef struct tcpck_conn_table tcpck_conn_table;
int tcpck_conn_table_create(tcpck_ctx *ctx, uint32_t max_conns, tcpck_conn_table **out);
int tcpck_conn_table_destroy(tcpck_conn_table *t);
int tcpck_conn_table_set(tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip, uint16_t peer_port, uint32_t id);
int tcpck_conn_table_erase(tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip, uint16_t peer_port);
int tcpck_conn_table_find(const tcpck_conn_table *t, uint16_t host_port, uint32_t peer_ip, uint16_t peer_port, uint32_t *id);
int tcpck_conn_table_commit(tcpck_conn_table *t, tcpck_stream stream);
int tcpck_conn_table_stats(const tcpck_conn_table *t, uint64_t *slots, uint64_t *entries, uint32_t *longest_probe, uint64_t *wrapped);

/* The batched lookup.  d_hdr: the dense host-order header array of
 * tcpck_batch_receive (d_hdr != NULL there), 32 * count bytes, 4-B aligned:
 * the source address is the u32 at byte 0, the source and destination ports
 * the u16 at bytes 12 and 14, the flags byte 25 (ACK 0x08, SYN 0x40).
 * d_conn[k] (u32, 4-B aligned) = the id the committed table holds for image
 * k's key under the rules above, else TCPCK_CONN_NONE.  d_hdr is only read;
 * nothing past d_conn[count) is written.  Asynchronous on `stream`; nothing is
 * allocated; no host synchronisation.  count == 0 is TCPCK_OK.  TCPCK_EINVAL:
 * ctx or t NULL; a host-only table, a table of another device or one never
 * committed; with count > 0 a NULL or misaligned d_hdr or d_conn. */
int tcpck_batch_demux(tcpck_ctx *ctx, const tcpck_conn_table *t, const void *d_hdr, uint64_t count,
                      uint32_t *d_conn, tcpck_stream stream);

/* The host planner over a mixed ring: tcpck_plan_deliver for every connection
 * of the ring at once, in ring order.  h_hdr, h_ok, h_lengths / len as in
 * tcpck_plan_deliver; h_conn[k]: image k's connection, TCPCK_CONN_NONE or an
 * index into conns[0, n_conns) (the ids of the connection table are these
 * indices).  conns[c].rcv is the connection's control block, conns[c].recv_base
 * / recv_bytes its window of one shared receive buffer (rcv.delivered counts
 * within the window); disjoint windows are the caller's precondition.
 * Every conns[c].stopped_at is set to TCPCK_NOT_STOPPED on entry.  Image k, c
 * = h_conn[k]:
 *   c == NONE       no socket (socket-manager.h:197-207): h_dst[k] = SKIP; bad
 *                   sum: verdict 0, h_ack[k] = 0; good sum: TCPCK_RCV_RST,
 *                   h_ack[k] = the image's acknowledgement number (header
 *                   bytes 20-23), the RST's sequence number -- but once an
 *                   earlier image of this call got TCPCK_RCV_HOST, a good-sum
 *                   unknown image gets TCPCK_RCV_HOST (h_ack[k] = 0): a SYN
 *                   handed to a listener makes the reference insert a new
 *                   socket (InternalNewConnection, socket-manager.h:70-90)
 *                   that later packets of that peer find and the committed
 *                   table cannot know, so the host looks those up again;
 *   CONN_HOST set   TCPCK_RCV_HOST, SKIP, h_ack[k] = conns[c].rcv.rcv_nxt, no
 *                   state change: listeners, handshakes, closing connections;
 *   c stopped       verdict 0, SKIP, h_ack[k] = rcv_nxt (what
 *                   tcpck_plan_deliver writes from `consumed` on);
 *   otherwise       exactly one step of tcpck_plan_deliver on conns[c].rcv
 *                   against conns[c].recv_bytes (the same code); an appended
 *                   payload gets h_dst[k] = recv_base + rcv.delivered,
 *                   absolute in the shared buffer.  Where the single planner
 *                   would stop (a FIN in sequence, a payload that does not
 *                   fit) only this connection stops: stopped_at = k, verdict
 *                   0, SKIP, h_ack[k] = rcv_nxt; the others go on.
 * The result feeds tcpck_batch_deliver unchanged: one launch over the ring,
 * d_recv the shared buffer, recv_bytes its whole size.  TCPCK_EINVAL, nothing
 * written: with count > 0 a NULL h_hdr, h_ok, h_conn, h_dst, h_verdict or
 * h_ack; n_conns > 0 and conns NULL; a bad length (as tcpck_plan_deliver); an
 * h_conn[k] neither TCPCK_CONN_NONE nor < n_conns; an odd recv_base;
 * recv_base + recv_bytes overflowing; rcv.delivered > recv_bytes. */
#define TCPCK_CONN_ESTAB 0u       /* planned here by Estab's rule */
#define TCPCK_CONN_HOST 1u        /* listener, handshake, closing: every image goes to the host state machine */
#define TCPCK_NOT_STOPPED UINT64_MAX
#define TCPCK_RCV_RST 16u         /* no socket, good sum: reply RST, seq = h_ack[k] (the image's ack number) */
#define TCPCK_RCV_HOST 32u        /* not decided here: run this image through the host path, in arrival order */
typedef struct tcpck_conn_state {
  tcpck_rcv_state rcv;            /* as tcpck_plan_deliver; rcv.delivered counts within this window */
  uint64_t recv_base, recv_bytes; /* this connection's window of the shared receive buffer; recv_base even */
  uint64_t stopped_at;            /* out: TCPCK_NOT_STOPPED, or the ring index where this connection's walk stopped */
  uint32_t flags, reserved;
} tcpck_conn_state;
int tcpck_plan_deliver_multi(const void *h_hdr, const uint8_t *h_ok, const uint32_t *h_conn,
                             const uint32_t *h_lengths, uint32_t len, uint64_t count,
                             tcpck_conn_state *conns, uint32_t n_conns,
                             uint64_t *h_dst, uint8_t *h_verdict, uint32_t *h_ack);

/* ---- batched replies: the planners' verdicts -> the ACK / RST ring ---------
 * What the reference sends back for a received datagram, for a whole ring:
 *   ACK  SocketInternal::SendAck (include/socket-internal.h:293-299):
 *        MakeTcpPacket(0), AckHeader(seq, ack, wnd) sets the ACK bit, seq, ack
 *        and window; SocketInternal::SendPacket (src/socket-internal.cc:35-42)
 *        SetSource / SetDestination and TcpHeaderH2N; SocketManager::SendPacket
 *        (src/socket-manager.cc:6-12) Checksum() = 0, then the checksum.  The
 *        call sites are Estab's data branch (src/state.cc:203-210) and
 *        InvalideCheckSum (include/state.h:268-275): seq = snd_nxt, wnd =
 *        snd_wnd in both;
 *   RST  for a datagram of no socket (ReceivePacket,
 *        include/socket-manager.h:201-207): MakeTcpPacket(0), RstHeader sets
 *        the RST bit and seq = the packet's acknowledgement number,
 *        TcpHeaderH2N, the checksum -- and NO SetSource / SetDestination: this
 *        RST leaves with zero addresses and ports, which is kept.
 * The reference's packet constructor leaves every byte the helpers do not set
 * (8-11, 24, the other bits of 25, 30-31) as the heap held it; here an ACK
 * takes them from the connection's template and an RST has them zero.
 *
 * d_verdict[k], d_ack[k]: the planner's h_verdict / h_ack (tcpck_plan_deliver,
 * tcpck_plan_deliver_multi), uploaded by the caller.  d_conn[k]: image k's
 * connection (tcpck_batch_demux's ids); NULL: every image is connection 0.
 * d_tmpl: one 32-B network-order header per connection, 32 * n_conns bytes --
 * the same kind of header tcpck_batch_segment takes as `hdr`, with bytes 16-19
 * = htonl(snd_nxt) and 26-27 = htons(snd_wnd); keeping snd_nxt current there
 * is the caller's (4 bytes per connection that sent).  Per image k, c =
 * d_conn ? d_conn[k] : 0:
 *   verdict & TCPCK_RCV_RST           32 zero bytes, bytes 16-19 :=
 *                                     htonl(d_ack[k]), byte 25 := 0x20; c is
 *                                     not looked at;
 *   else verdict & TCPCK_RCV_SEND_ACK and c < n_conns
 *                                     template c, bytes 20-23 :=
 *                                     htonl(d_ack[k]), byte 25 |= 0x08;
 *   else                              no reply (TCPCK_RCV_HOST, verdict 0,
 *                                     SEND_ACK with c == TCPCK_CONN_NONE or c
 *                                     >= n_conns: no template is read outside
 *                                     [0, n_conns), whatever the arrays hold).
 * Bytes 28-29 of every reply end as tcpck_fill16(image, 32, mode) leaves them
 * (both modes).  Reply j goes to d_replies + 32 j: dense and in ring order, the
 * j-th reply answers the j-th replying image (the reference replies in arrival
 * order); d_src[j] = k (d_src may be NULL); *d_count (device, u64) = the number
 * of replying images.  When that exceeds reply_cap only the first reply_cap
 * replies and d_src entries are written and *d_count still holds the total.
 * Nothing is written past d_replies[32 * min(total, reply_cap)) or
 * d_src[min(total, reply_cap)); the inputs are only read.  d_scratch: device
 * memory of the size tcpck_reply_scratch_bytes(count, &bytes) gives (never 0),
 * its contents undefined before and after.  Asynchronous on `stream`; nothing
 * is allocated; no host synchronisation; the same inputs give the same bytes.
 * count == 0 is TCPCK_OK and sets *d_count = 0 in stream order when d_count is
 * not NULL.  TCPCK_EINVAL, nothing launched: ctx NULL; a bad mode; count >
 * 2^31; with count > 0 a NULL d_verdict, d_ack, d_replies, d_count or
 * d_scratch; n_conns > 0 with d_tmpl NULL; a misaligned pointer (d_ack, d_conn,
 * d_src 4-B; d_tmpl, d_replies, d_scratch 16-B; d_count 8-B).
 * tcpck_reply_scratch_bytes: TCPCK_EINVAL for bytes NULL or count > 2^31. */
#define TCPCK_REPLY_BYTES 32
int tcpck_reply_scratch_bytes(uint64_t count, size_t *bytes);
int tcpck_batch_reply(tcpck_ctx *ctx, int mode, const uint8_t *d_verdict, const uint32_t *d_ack,
                      const uint32_t *d_conn, const void *d_tmpl, uint32_t n_conns, uint64_t count,
                      void *d_replies, uint64_t reply_cap, uint32_t *d_src, uint64_t *d_count,
                      void *d_scratch, tcpck_stream stream);
/* The same contract on host arrays: plain host C++, reentrant, no device, no
 * scratch; the number of replying images is returned through n_replies.  The
 * CPU fallback and the second implementation the device call is tested
 * against.  Nothing is written on an error. */
int tcpck_build_replies(int mode, const uint8_t *h_verdict, const uint32_t *h_ack, const uint32_t *h_conn,
                        const void *h_tmpl, uint32_t n_conns, uint64_t count,
                        void *h_replies, uint64_t reply_cap, uint32_t *h_src, uint64_t *n_replies);

/* ---- batched segmentation: send stream -> checksummed images -------------
 * The data-segment send path in one device pass.  The reference, per segment:
 * TcpSendingBuffer::GetAsTcpPacket(0, window) cuts the next <= window bytes
 * off the send stream into a fresh packet with TcpLength = len
 * (include/tcp-buffer.h:82-98); Estab sets ACK, seq = snd_nxt (then snd_nxt
 * += len) and ack (src/state.cc:167-184); SetSource/SetDestination and
 * TcpHeaderH2N (include/socket-internal.h:186-199); SendPacketsForSending
 * zeroes and stores the checksum (include/socket-manager.h:259-260).  Here:
 *   n = ceil(payload_bytes / seg) images, image k at d_images + k * stride:
 *     bytes 0-31  = hdr (a 32-B network-order header: the connection's fields
 *                   as TcpHeaderH2N leaves them) with TcpLength (10-11) =
 *                   htons(len_k), seq (16-19) = htonl(seq0 + k * seg) and the
 *                   checksum (28-29) of the image (raw, as the reference);
 *     bytes 32..  = d_payload[k * seg, k * seg + len_k), len_k = seg except
 *                   the last (the rest); the slot's bytes after the image = 0.
 * payload_bytes even; seg a multiple of 4 in [4, 65532]; stride a multiple of
 * 16, >= 32 + seg; d_payload 4-B and d_images 16-B aligned; hdr a host pointer
 * (read during the call).  d_out: u16[n] checksums (may be NULL).  Both modes
 * (RFC 1071 folds the same sums).  Asynchronous on `stream`. */
int tcpck_batch_segment(tcpck_ctx *ctx, int mode, const void *d_payload, uint64_t payload_bytes,
                        uint32_t seg, const void *hdr, uint32_t seq0, void *d_images, uint64_t stride,
                        uint16_t *d_out, tcpck_stream stream);

/* ---- batched, host memory (end to end incl. PCIe) ------------------------
 * Segments start and end in host memory (the loopback/socket buffers of
 * network-service.cc / tcp-buffer.h).  The batch is split into chunks that are
 * streamed H2D -> kernel -> D2H on two ctx-owned HIP streams with ctx-owned
 * device staging buffers.  Synchronous: returns when h_out (and, for FILL,
 * h_arena) hold the results.  Host buffers should be pinned
 * (tcpck_host_alloc) for full PCIe rate.  offsets/lengths are host arrays. */
int tcpck_host_batch_fixed(tcpck_ctx *ctx, int op, int mode, void *h_arena,
                           uint64_t stride, uint32_t len, uint64_t count,
                           void *h_out);
int tcpck_host_batch_var(tcpck_ctx *ctx, int op, int mode, void *h_arena,
                         const uint64_t *h_offsets, const uint32_t *h_lengths,
                         uint64_t count, void *h_out);
/* The same host batch over several contexts at once -- one per GPU of the
 * node, each with its own PCIe link (independent segments, no
 * exchange step): contiguous shards, equal image counts (fixed) or balanced by
 * bytes (variable, over h_lengths), each run by tcpck_host_batch_* on its own
 * host thread (the first on the calling thread).  Results land in h_out by
 * index as from one context.  Synchronous; returns the first failing shard's
 * status.  A context listed twice runs its shards one after the other. */
int tcpck_host_batch_fixed_multi(tcpck_ctx *const *ctxs, int n_ctx, int op, int mode, void *h_arena,
                                 uint64_t stride, uint32_t len, uint64_t count, void *h_out);
int tcpck_host_batch_var_multi(tcpck_ctx *const *ctxs, int n_ctx, int op, int mode, void *h_arena,
                               const uint64_t *h_offsets, const uint32_t *h_lengths, uint64_t count,
                               void *h_out);
/* Bytes of device staging per chunk used by the host batch functions. */
int tcpck_ctx_set_chunk_bytes(tcpck_ctx *ctx, uint64_t bytes);

/* ---- memory helpers (for C/C++ callers without another allocator) -------- */
int tcpck_host_alloc(size_t bytes, void **out);   /* pinned host memory   */
int tcpck_host_free(void *p);
int tcpck_device_alloc(tcpck_ctx *ctx, size_t bytes, void **out);
int tcpck_device_free(tcpck_ctx *ctx, void *p);
int tcpck_memcpy_h2d(tcpck_ctx *ctx, void *dst, const void *src, size_t bytes);
int tcpck_memcpy_d2h(tcpck_ctx *ctx, void *dst, const void *src, size_t bytes);
int tcpck_stream_sync(tcpck_ctx *ctx, tcpck_stream stream);

/* ---- synthetic workload generator (benchmarks/tests; not the hot path) ----
 * Writes images with the send path's 32-byte header (127.0.0.1:15500 ->
 * 127.0.0.1:15501, PTCL 6, TcpLength = payload, seq = 1000 + index, ACK,
 * window 1024, network order, checksum 0) and a payload drawn from splitmix64
 * keyed by (seed, first_index + k) -- any shard is reproducible on its own.
 * kind: 0 random payload, 1 all-zero payload, 2 all-0xFF payload. */
int tcpck_synth_fixed(void *d_arena, uint64_t stride, uint32_t len, uint64_t count,
                      uint64_t seed, uint64_t first_index, int kind, tcpck_stream stream);
int tcpck_synth_var(void *d_arena, const uint64_t *d_offsets, const uint32_t *d_lengths,
                    uint32_t max_len, uint64_t count, uint64_t seed, uint64_t first_index,
                    int kind, tcpck_stream stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* TCPCK_H_ */
