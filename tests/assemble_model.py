"""Model of floria_hip_assemble_contigs for the tests: combine_frags (file_reader.rs:539-541, 636-639) stated on the per-record cells of
tests/pileup_model.py: walk_records.  A fragment is an ordered list of record indices; the later record's call overwrites the earlier one's
(`seq_dict.extend`), the cells ascend by SNP, first / last are the smallest / largest merged SNP, and the fragments of a contig are sorted by Frag::cmp
(first ascending, last descending, the fragment's place in the host's list).  Written with numpy sorting, not as the kernel does it (no windows, no
searches); tests/test_assemble_cpu.py checks it against a plain-dict restatement.

Also here: the helper that turns per-contig lists of fragments into a sorted floria_fragment_plan plus the equivalent Pileup objects, and a record builder
that puts chosen (SNP, allele, quality) cells into one alignment record."""
import numpy as np

from floria_amd.pileup import Pileup
from tests import pileup_model as pm


def record_cells(walked, i):
    cell_off, snp, allele, qual = walked[0], walked[1], walked[2], walked[3]
    a, b = int(cell_off[i]), int(cell_off[i + 1])
    return snp[a:b], allele[a:b], qual[a:b]


def merge_fragment(walked, parts):
    """parts: record indices in merge order -> (snp uint32, allele uint8, qual uint8) of the merged fragment, ascending by SNP"""
    cells = [record_cells(walked, i) for i in parts]
    s = np.concatenate([c[0] for c in cells] + [np.zeros(0, np.uint32)]).astype(np.int64)
    a = np.concatenate([c[1] for c in cells] + [np.zeros(0, np.uint8)])
    q = np.concatenate([c[2] for c in cells] + [np.zeros(0, np.uint8)])
    idx = np.lexsort((np.arange(len(s)), s))                  # by SNP, then by the order of insertion
    if len(idx) == 0:
        return s.astype(np.uint32), a, q
    ss = s[idx]
    keep = np.r_[ss[1:] != ss[:-1], True]                      # the LAST insertion of every SNP
    idx = idx[keep]
    return s[idx].astype(np.uint32), a[idx], q[idx]


def frag_order(firsts, lasts):
    """Frag::cmp (types_structs.rs:87-93) with counter_id = the place in the list"""
    f, l = np.asarray(firsts, np.int64), np.asarray(lasts, np.int64)
    return np.lexsort((np.arange(len(f)), -l, f))


def build_plan(walked, frags_per_contig, set_order_rng=None):
    """frags_per_contig: for every contig a list of fragments (lists of record indices, merge order), in ANY order
    -> dict(frag_off uint64, part_off uint64, part_rec uint32, set_order uint32 | None, pileups [Pileup per contig], order [the sort permutation per contig]).
    With set_order_rng every fragment gets a random permutation of its merged cells' indices, on the plan and on the pileups alike."""
    frag_off, part_off, part_rec, pileups, orders, so_all = [0], [0], [], [], [], []
    for frags in frags_per_contig:
        merged = [merge_fragment(walked, f) for f in frags]
        assert all(len(m[0]) for m in merged), "a fragment without cells cannot be part of a pileup"
        order = frag_order([m[0][0] for m in merged], [m[0][-1] for m in merged])
        orders.append(order)
        off, so = [0], []
        for k in order:
            part_rec += list(frags[k]); part_off.append(len(part_rec)); off.append(off[-1] + len(merged[k][0]))
            if set_order_rng is not None:
                so.append(set_order_rng.permutation(len(merged[k][0])).astype(np.uint32))
        cat = lambda j, dt: np.concatenate([merged[k][j] for k in order] + [np.zeros(0, dt)]).astype(dt)
        p = Pileup(np.asarray(off, np.uint32), cat(0, np.uint32), cat(1, np.uint8), cat(2, np.uint8),
                   np.asarray([merged[k][0][0] for k in order], np.uint32), np.asarray([merged[k][0][-1] for k in order], np.uint32))
        if set_order_rng is not None:
            p.set_order = np.concatenate(so + [np.zeros(0, np.uint32)]).astype(np.uint32)
            so_all.append(p.set_order)
        pileups.append(p)
        frag_off.append(frag_off[-1] + len(frags))
    return dict(frag_off=np.asarray(frag_off, np.uint64), part_off=np.asarray(part_off, np.uint64), part_rec=np.asarray(part_rec, np.uint32),
                set_order=np.concatenate(so_all + [np.zeros(0, np.uint32)]).astype(np.uint32) if set_order_rng is not None else None,
                pileups=pileups, order=orders)


# ---- records with chosen cells -------------------------------------------------------------------------------------------------------------------
BASES = b"ACGT"


def grid_table(n_snps, start=100, step=10):
    """SNPs every `step` bases; every site has the four alleles A C G T, so a read base IS its allele index"""
    return pm.SnpTable(start + step * np.arange(n_snps), np.tile(np.frombuffer(BASES, np.uint8), (n_snps, 1)), np.full(n_snps, 4, np.uint8))


def record_with(table, cells, contig=0, name="f"):
    """cells: {1-based SNP index: (allele, qual)} -> one alignment record (a single M run, N at every other base) whose walk yields exactly these cells;
    an empty dict gives a record that covers SNP 1 with an N: no cell"""
    snps = sorted(cells) if cells else [1]
    lo, hi = int(table.pos[snps[0] - 1]), int(table.pos[snps[-1] - 1])
    seq = bytearray(b"N" * (hi - lo + 1))
    qual = np.full(len(seq), 7, np.uint8)
    for s, (a, q) in cells.items():
        seq[int(table.pos[s - 1]) - lo] = BASES[a]; qual[int(table.pos[s - 1]) - lo] = q
    return pm.make_record(lo, [("M", len(seq))], bytes(seq), qual, contig=contig, name=name)
