"""Model of the read positions on resident contigs for the tests: Frag::snp_pos_to_seq_pos as one SEQ_POS word `mate << 31 | seq_pos` per cell, through the three
stages that touch it.

    merge     combine_frags (file_reader.rs:539-541, 636-639): `snp_pos_to_seq_pos.extend` follows the rule of `seq_dict.extend`, the later part's entry
              overwrites the earlier one's — tests/assemble_model.py: merge_fragment with the word as a fourth column;
    filter    remove_monomorphic_allele removes the key with the cell (utils_frags.rs:749) — tests/mono_model.py: drop_monomorphic's survivor mask and old_read;
    query     write_reads (file_writer.rs:460-530): the entry of the read's first SNP at or behind the haploset's left end and of its last SNP at or before its
              right end — np.searchsorted over the read's ascending SNPs.

Written with numpy sorting and searching, not as the kernels do it; tests/test_span_cpu.py checks it against a plain-dict restatement and the C++ host."""
import numpy as np

from tests import mono_model as mm

NONE = 0xFFFFFFFF


def word(mate, seq_pos):
    return (np.asarray(mate, np.uint32) << np.uint32(31)) | np.asarray(seq_pos, np.uint32)


def merge_seq_pos(walked, parts, part_mate=None):
    """parts: record indices in merge order, part_mate: 0 / 1 per part (None = all 0) -> (snp uint32, allele uint8, qual uint8, word uint32) of the merged
    fragment, ascending by SNP"""
    cell_off = walked[0]
    mates = np.zeros(len(parts), np.uint32) if part_mate is None else np.asarray(part_mate, np.uint32)
    cols = [[], [], [], []]
    for i, m in zip(parts, mates):
        a, b = int(cell_off[i]), int(cell_off[i + 1])
        cols[0].append(walked[1][a:b]); cols[1].append(walked[2][a:b]); cols[2].append(walked[3][a:b]); cols[3].append(word(np.full(b - a, m, np.uint32), walked[4][a:b]))
    s = np.concatenate(cols[0] + [np.zeros(0, np.uint32)]).astype(np.int64)
    a = np.concatenate(cols[1] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    q = np.concatenate(cols[2] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    w = np.concatenate(cols[3] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    idx = np.lexsort((np.arange(len(s)), s))                  # by SNP, then by the order of insertion
    if len(idx):
        ss = s[idx]
        idx = idx[np.r_[ss[1:] != ss[:-1], True]]             # the LAST insertion of every SNP
    return s[idx].astype(np.uint32), a[idx], q[idx], w[idx]


def later_parts_mate(plan):
    """part_mate [n_parts] that marks every part after a fragment's first"""
    pm = np.ones(len(plan["part_rec"]), np.uint8)
    pm[plan["part_off"][:-1].astype(np.int64)] = 0
    return pm


def plan_words(walked, plan, part_mate=None):
    """the SEQ_POS words of every contig of a plan of tests/assemble_model.py: build_plan -> [uint32 [n_cells] per contig]"""
    po, fo = plan["part_off"].astype(np.int64), plan["frag_off"].astype(np.int64)
    out = []
    for c in range(len(fo) - 1):
        ws = []
        for f in range(fo[c], fo[c + 1]):
            parts = plan["part_rec"][po[f]:po[f + 1]]
            s, _, _, w = merge_seq_pos(walked, parts, None if part_mate is None else part_mate[po[f]:po[f + 1]])
            ws.append(w)
        out.append(np.concatenate(ws + [np.zeros(0, np.uint32)]).astype(np.uint32))
        assert len(out[-1]) == plan["pileups"][c].n_cells
    return out


def filter_words(p, words, n_snps, error):
    """the words of mono_model.drop_monomorphic(p, n_snps, error)'s pileup: the survivors', in the order of its reads"""
    q, old_read, removed = mm.drop_monomorphic(p, n_snps, error)
    keep = removed[p.snp.astype(np.int64) - 1] == 0 if p.n_cells else np.zeros(0, bool)
    ws = []
    for r in old_read:
        lo, hi = int(p.read_off[r]), int(p.read_off[r + 1])
        ws.append(words[lo:hi][keep[lo:hi]])
    out = np.concatenate(ws + [np.zeros(0, np.uint32)]).astype(np.uint32)
    assert len(out) == q.n_cells
    return q, out


def read_spans(pileups, words, grp_contig, groups, ranges):
    """floria_hip_read_spans -> (left uint32, right uint32), one entry per read of every group"""
    left, right = [], []
    for c, grp, (lo, hi) in zip(grp_contig, groups, ranges):
        p, w = pileups[c], words[c]
        for r in grp:
            b, e = int(p.read_off[r]), int(p.read_off[r + 1])
            s = p.snp[b:e].astype(np.int64)
            i, k = int(np.searchsorted(s, int(lo), "left")), int(np.searchsorted(s, int(hi), "right"))
            left.append(int(w[b + i]) if i < e - b else NONE)
            right.append(int(w[b + k - 1]) if k > 0 else NONE)
    return np.asarray(left, np.uint32), np.asarray(right, np.uint32)
