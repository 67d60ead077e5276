"""What an index-driven read of a BAM can at best do, computed from the BAM alone with Python's zlib: for every target the virtual offset of its first record
and the set of BGZF members that hold at least one byte of its records.  Independent of floria_amd/host/ingest.cpp and of synth_bam.write_bai; the tests
compare both with it.  Also a reader of the per-target begins of a .bai file (SAM specification 5.2), for indexes written by any program."""
import struct
import zlib


def members(path):
    """-> [(file offset, compressed size, inflated bytes)] of every BGZF member"""
    packed = open(path, "rb").read()
    out, o = [], 0
    while o < len(packed):
        assert packed[o:o + 4] == b"\x1f\x8b\x08\x04", f"no BGZF member at byte {o} of {path}"
        xlen, = struct.unpack_from("<H", packed, o + 10)
        x, bsize = o + 12, None
        while x + 4 <= o + 12 + xlen:
            s1, s2, slen = struct.unpack_from("<BBH", packed, x)
            if (s1, s2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", packed, x + 4)[0] + 1
            x += 4 + slen
        assert bsize is not None
        data = zlib.decompressobj(-15).decompress(packed[o + 12 + xlen:o + bsize - 8])
        assert len(data) == struct.unpack_from("<I", packed, o + bsize - 4)[0]
        out.append((o, bsize, data))
        o += bsize
    return out


def model(path):
    """-> dict(n_ref, names, n_members, begin={tid: virtual offset of its first record}, members={tid: set of member file offsets holding a byte of its
    records}, n_records={tid: count}, n_unplaced)"""
    mem = members(path)
    raw = b"".join(m[2] for m in mem)
    owner = []                                          # inflated byte -> index of its member
    for k, m in enumerate(mem):
        owner.extend([k] * len(m[2]))
    start_of = []
    acc = 0
    for m in mem:
        start_of.append(acc)
        acc += len(m[2])
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, o)
    o += 4
    names = []
    for _ in range(n_ref):
        ln, = struct.unpack_from("<I", raw, o)
        names.append(raw[o + 4:o + 4 + ln - 1].decode())
        o += 4 + ln + 4
    begin, held, count, unplaced = {}, {}, {}, 0
    while o < len(raw):
        bs, tid = struct.unpack_from("<Ii", raw, o)
        if tid < 0:
            unplaced += 1
        else:
            if tid not in begin:
                k = owner[o]
                begin[tid] = (mem[k][0] << 16) | (o - start_of[k])
            held.setdefault(tid, set()).update(mem[owner[p]][0] for p in range(o, o + 4 + bs))
            count[tid] = count.get(tid, 0) + 1
        o += 4 + bs
    assert o == len(raw)
    return dict(n_ref=n_ref, names=names, n_members=len(mem), begin=begin, members=held, n_records=count, n_unplaced=unplaced)


def bai_begins(path):
    """-> ({tid: smallest chunk begin over the real bins}, {tid: ref_beg of the pseudo-bin 37450 where there is one}, n_ref)"""
    b = open(path, "rb").read()
    assert b[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<I", b, 4)
    o = 8
    begins, pseudo = {}, {}
    for tid in range(n_ref):
        n_bin, = struct.unpack_from("<I", b, o)
        o += 4
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<II", b, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", b, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            if bin_ == 37450:
                pseudo[tid] = chunks[0][0]
            else:
                for beg, _end in chunks:
                    begins[tid] = min(begins.get(tid, beg), beg)
        n_intv, = struct.unpack_from("<I", b, o)
        o += 4 + 8 * n_intv
    assert o in (len(b), len(b) - 8)
    return begins, pseudo, n_ref
