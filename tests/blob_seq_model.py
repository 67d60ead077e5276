"""The numpy model of floria_hip_blob_sequences: what frag_sequences (host/ingest.cpp) makes of a record's packed bases and quality bytes.
  base     the 4-bit code 1 / 2 / 4 / 8 is A / C / G / T, every other code is A; the high nibble of a byte comes first, the partner of an odd length's last nibble is padding
  quality  q > 222 ? 255 : q + 33"""
import numpy as np

LETTER = np.full(16, ord("A"), np.uint8)
LETTER[[1, 2, 4, 8]] = np.frombuffer(b"ACGT", np.uint8)


def bases(packed, l_seq):
    """packed: the (l_seq + 1) // 2 bytes of a record's sequence -> l_seq letters"""
    p = np.asarray(packed, np.uint8)
    nib = np.empty(2 * len(p), np.uint8)
    nib[0::2] = p >> 4
    nib[1::2] = p & 15
    return LETTER[nib[:l_seq]]


def quals(q):
    q = np.asarray(q, np.uint8).astype(np.uint16)
    return np.where(q > 222, 255, q + 33).astype(np.uint8)


def sequences(raw, seq_off, l_seq, qual_off):
    """the whole call: (base_off [n + 1], bases, quals) for records given as offsets into the bytes `raw`"""
    raw = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray)) else np.asarray(raw, np.uint8)
    base_off = np.concatenate([[0], np.cumsum(np.asarray(l_seq, np.uint64))]).astype(np.uint64)
    b = [bases(raw[int(s):int(s) + (int(n) + 1) // 2], int(n)) for s, n in zip(seq_off, l_seq)]
    q = [quals(raw[int(o):int(o) + int(n)]) for o, n in zip(qual_off, l_seq)]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return base_off, cat(b), cat(q)
