"""What tcpck_segment_headers / tcpck_batch_segment_headers must produce for a planned send ring,
from oracle.ref16.segment_np applied per cut: bytes 0-31 of every image, where its payload lies,
and its checksum.  Shared by tests/test_segment_headers.py and tests/test_gpu_segment_headers.py."""
import numpy as np

from oracle.ref16 import segment_np


def make_cuts(sizes, seqs, tmpls, residues=(0,)):
    """An unplanned cut table (tcpck.send_cut_dtype()) and the arena size: cut c of sizes[c] bytes,
    laid one after the other, its offset congruent to residues[c % len(residues)] mod 16."""
    import tcpck
    cuts = np.zeros(len(sizes), tcpck.send_cut_dtype())
    at = 0
    for c, n in enumerate(sizes):
        at += (residues[c % len(residues)] - at) % (16 if len(residues) > 1 else 4)
        cuts[c]["offset"], cuts[c]["bytes"], cuts[c]["seq0"], cuts[c]["tmpl"] = at, n, seqs[c], tmpls[c]
        at += n
    return cuts, at + (-at) % 2


def ring_np(payload, cuts, tmpl, seg, n_seg, mode=0, skip=()):
    """(hdr u8[n_seg, 32], pay_off u64, pay_len u32, checksums u16) of the planned table `cuts`;
    the cuts in `skip` claim nothing: their segments stay zero."""
    hdr = np.zeros((n_seg, 32), np.uint8)
    off, ln, cs = np.zeros(n_seg, np.uint64), np.zeros(n_seg, np.uint32), np.zeros(n_seg, np.uint16)
    for c, cut in enumerate(cuts):
        o, b, f = int(cut["offset"]), int(cut["bytes"]), int(cut["first"])
        if c in skip or b == 0:
            continue
        imgs, lens, csum = segment_np(payload[o:o + b], seg, tmpl[int(cut["tmpl"])], int(cut["seq0"]), mode=mode)
        n = lens.size
        hdr[f:f + n] = imgs.reshape(n, 32 + seg)[:, :32]
        off[f:f + n] = o + np.arange(n, dtype=np.uint64) * seg
        ln[f:f + n] = lens - 32
        cs[f:f + n] = csum
    return hdr, off, ln, cs
