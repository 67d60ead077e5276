"""The DEFLATE cases of the device inflater (csrc/inflate_kernel.h), shared by the CPU check of its decoder core (tests/test_inflate_core_cpu.py) and the GPU tests
(tests/test_gpu_inflate.py).  zlib of the standard library is the generator and the model; the cases zlib's compressor never writes are assembled bit by bit here.

A case is (name, payload, isize, status): `payload` raw DEFLATE, `isize` the output length the member claims, `status` the INF_* word the decoder must end with
(0: the output equals zlib.decompress(payload, -15))."""
import struct
import zlib

import numpy as np

from floria_amd import synth_bam

STATUS = {"ok": 0, "bits ran out": 1, "reserved block type": 2, "LEN/NLEN mismatch": 3, "over-subscribed code lengths": 4, "incomplete code lengths": 5,
          "distance beyond the bytes produced": 6, "output longer than ISIZE": 7, "output shorter than ISIZE": 8, "CRC mismatch": 9, "invalid code": 10}
BGZF_MAX = 65280


class Bits:
    """DEFLATE's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.put(int(format(c, f"0{n}b")[::-1], 2), n)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def fixed_block(ops, final=True):
    """one fixed-Huffman block from literals (ints) and matches ((length, distance) pairs)"""
    b = Bits()
    b.put(1 if final else 0, 1); b.put(1, 2)

    def sym(s):
        if s < 144: b.code(0x30 + s, 8)
        elif s < 256: b.code(0x190 + s - 144, 9)
        elif s < 280: b.code(s - 256, 7)
        else: b.code(0xC0 + s - 280, 8)
    for op in ops:
        if isinstance(op, tuple):
            ln, dist = op
            i = max(k for k in range(29) if _LBASE[k] <= ln) if ln != 258 else 28
            sym(257 + i); b.put(ln - _LBASE[i], _LEXT[i])
            j = max(k for k in range(30) if _DBASE[k] <= dist)
            b.code(j, 5); b.put(dist - _DBASE[j], _DEXT[j])
        else:
            sym(op)
    sym(256)
    return b.done()


def repeat_codes_block():
    """a dynamic block whose header uses the repeat codes 16, 17 and 18, the 16 running from the last literal/length lengths into the distance lengths:
    literal/length symbols 65, 66, 256 and 257 and the four distance symbols all have two-bit codes"""
    b = Bits()
    b.put(1, 1); b.put(2, 2)
    b.put(258 - 257, 5); b.put(4 - 1, 5); b.put(16 - 4, 4)
    cl = {16: 2, 17: 2, 18: 2, 2: 2}
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2):
        b.put(cl.get(s, 0), 3)
    c2, c16, c17, c18 = 0, 1, 2, 3                                   # canonical: ascending symbols of one length
    b.code(c18, 2); b.put(65 - 11, 7)                                # lengths 0 .. 64: zero
    b.code(c2, 2); b.code(c2, 2)                                     # 65, 66
    b.code(c18, 2); b.put(138 - 11, 7); b.code(c18, 2); b.put(48 - 11, 7); b.code(c17, 2); b.put(3 - 3, 3)      # 67 .. 255: zero
    b.code(c2, 2)                                                    # 256
    b.code(c16, 2); b.put(5 - 3, 2)                                  # 257 and the four distance lengths: the repeat crosses from one alphabet into the other
    A, B, EOB, M3 = 0, 1, 2, 3
    for s in (A, B, A): b.code(s, 2)
    b.code(M3, 2); b.code(2, 2)                                      # length 3, distance 3
    b.code(M3, 2); b.code(0, 2)                                      # length 3, distance 1
    b.code(EOB, 2)
    return b.done()


def record_bytes(n_bytes, seed=3):
    """BAM alignment records as synth_bam writes them, cut at n_bytes"""
    rng = np.random.default_rng(seed)
    out, size, pos = [], 0, 1000
    while size < n_bytes:
        n = int(rng.integers(80, 900))
        pos += int(rng.integers(1, 300))
        r = synth_bam.bam_record(0, pos, f"read{len(out)}", 0, 60, [("M", n)], bytes(synth_bam.BASES[rng.integers(0, 4, size=n)]), rng.integers(5, 41, size=n).astype(np.uint8))
        out.append(r); size += len(r)
    return b"".join(out)[:n_bytes]


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw DEFLATE of `data`; flushes: (offset, mode) pairs at which the stream is flushed"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += c.compress(data[at:off]) + c.flush(mode); at = off
    return out + c.compress(data[at:]) + c.flush()


def fibonacci_bytes():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, 40 + i, np.uint8) for i, f in enumerate(fib)])
    np.random.default_rng(1).shuffle(data)
    return data.tobytes()


def valid_cases():
    rec = record_bytes(BGZF_MAX)
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, size=BGZF_MAX, dtype=np.uint8).tobytes()
    far = [int(x) for x in noise[:32768]]
    for _ in range((BGZF_MAX - 32768) // 258):
        far.append((258, 32768))
    far += [0] * ((BGZF_MAX - 32768) % 258)
    cases = [
        ("empty", deflate(b""), None),
        ("stored_65280", deflate(noise, 0), None),
        ("stored_len0_sync_flush", deflate(b"abc", 6, flushes=[(3, zlib.Z_SYNC_FLUSH)]), None),
        ("fixed_256_literals", fixed_block(list(range(256))), None),
        ("fixed_zlib", deflate(rec[:3000], 6, zlib.Z_FIXED), None),
        ("fixed_len3_len258", fixed_block([1, 2, 3, (3, 3)] + list(range(200)) * 2 + [(258, 300), (258, 258)]), None),
        ("fixed_dist1_len258", fixed_block([7, (258, 1), (258, 1), (5, 1)]), None),
        ("fixed_source_first_byte", fixed_block([9, 8, 7, 6, (4, 4), (3, 8), (258, 11)]), None),
        ("fixed_dist32768", fixed_block(far), None),
        ("dynamic_level1", deflate(rec, 1), None),
        ("dynamic_level6", deflate(rec, 6), None),
        ("dynamic_level9", deflate(rec, 9), None),
        ("huffman_only", deflate(rec[:20000], 6, zlib.Z_HUFFMAN_ONLY), None),
        ("rle", deflate(rec[:20000], 6, zlib.Z_RLE), None),
        ("one_distinct_byte", deflate(b"\x55" * 40000, 6), None),
        ("one_distinct_byte_huffman_only", deflate(b"\x55" * 5000, 6, zlib.Z_HUFFMAN_ONLY), None),
        ("fibonacci_lengths_to_15", deflate(fibonacci_bytes(), 9, zlib.Z_HUFFMAN_ONLY), None),
        ("repeat_codes_across_alphabets", repeat_codes_block(), None),
        ("blocks_sync_and_full_flush", deflate(rec[:6000] + rec[:6000] + rec[6000:9000], 6, flushes=[(6000, zlib.Z_SYNC_FLUSH), (12000, zlib.Z_FULL_FLUSH)]), None),
        ("one_byte", deflate(b"x"), None),
        ("three_bytes", deflate(b"xyz"), None),
    ]
    out = []
    for name, payload, _ in cases:
        out.append((name, payload, len(zlib.decompress(payload, -15)), 0))
    return out


def malformed_cases():
    rec = record_bytes(5000)
    good = deflate(rec, 6)
    over = Bits()
    over.put(1, 1); over.put(2, 2); over.put(0, 5); over.put(0, 5); over.put(0, 4)
    for l in (1, 1, 1, 0):
        over.put(l, 3)
    over.put(0, 32)
    stored = bytes([1]) + struct.pack("<HH", 5, 5 ^ 0xffff ^ 0x0100) + b"hello"
    return [
        ("truncated_payload", good[:len(good) // 2], len(rec), STATUS["bits ran out"]),
        ("block_type_3", bytes([0x07, 0, 0, 0]), 0, STATUS["reserved block type"]),
        ("len_nlen_mismatch", stored, 5, STATUS["LEN/NLEN mismatch"]),
        ("oversubscribed_lengths", over.done(), 0, STATUS["over-subscribed code lengths"]),
        ("distance_one_beyond", fixed_block([65, (3, 2)]), 4, STATUS["distance beyond the bytes produced"]),
        ("isize_one_too_small", good, len(rec) - 1, STATUS["output longer than ISIZE"]),
        ("isize_one_too_large", good, len(rec) + 1, STATUS["output shorter than ISIZE"]),
    ]


def bgzf_member(payload, data=None, isize=None, crc=None, extra=b"", magic=b"\x1f\x8b\x08\x04", bsize=None, bc=b"BC"):
    """one BGZF member around a raw DEFLATE payload; `extra`: subfields that stand before BC"""
    if data is None:
        data = zlib.decompress(payload, -15)
    xlen = len(extra) + 6
    total = 12 + xlen + len(payload) + 8
    head = magic + struct.pack("<IBBH", 0, 0, 255, xlen) + extra + bc + struct.pack("<HH", 2, (total if bsize is None else bsize) - 1)
    return head + payload + struct.pack("<II", (zlib.crc32(data) & 0xffffffff) if crc is None else crc, len(data) if isize is None else isize)


def write_case_file(path, cases):
    with open(path, "w") as f:
        for name, payload, isize, status in cases:
            f.write(f"{name} {status} {isize} {payload.hex() or '-'}\n")
