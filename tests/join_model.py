"""numpy model of floria_hip_join_paths: the union that ends get_disjoint_paths_rewrite (host/stitch.cpp).  A path is a list of hap-graph nodes (block, partition)
of one S1 batch; its haploset holds, ascending and once each, every read some node (b, k) of it lists in block b with part == k.

The S1 batch is given as floria_block_result gives it (read_off [n_blocks + 1], read_id, part); join() is the definition the GPU tests compare the download with,
node_reads() one node's set, and parse_stitch() / join_stitch() the same union on the text `floria-hip --stitch-graph --stitch-paths` prints (N lines: the nodes'
reads, Q lines: the paths' nodes), which tests/test_join_cpu.py pins to the P lines of the C++ host."""
import numpy as np


def node_reads(read_off, read_id, part, b, k):
    lo, hi = int(read_off[b]), int(read_off[b + 1])
    return np.asarray(read_id[lo:hi])[np.asarray(part[lo:hi]) == k]


def join(read_off, read_id, part, nodes):
    """nodes: per path a sequence of (block, partition) -> per path a sorted uint32 array without repeats."""
    out = []
    for path in nodes:
        sets = [node_reads(read_off, read_id, part, int(b), int(k)) for b, k in path]
        out.append(np.unique(np.concatenate(sets)).astype(np.uint32) if sets else np.zeros(0, np.uint32))
    return out


def windows(read_off, read_id, nodes):
    """Per path the id window [lo, hi) the kernels mark in: from the smallest first entry to the largest last entry + 1 of its nodes' block lists (0, 0 if none)."""
    out = []
    for path in nodes:
        lo, hi = None, 0
        for b, _ in path:
            a, z = int(read_off[b]), int(read_off[b + 1])
            if z > a:
                lo = int(read_id[a]) if lo is None else min(lo, int(read_id[a]))
                hi = max(hi, int(read_id[z - 1]) + 1)
        out.append((0, 0) if lo is None else (lo, hi))
    return out


def candidates(groups, n_reads):
    """Number of groups every read sits in."""
    c = np.zeros(n_reads, np.int64)
    for g in groups:
        c[np.asarray(g, np.int64)] += 1
    return c


def parse_stitch(text):
    """N / Q / P lines of `floria-hip --stitch-graph FILE --stitch-paths` (the input file's N lines followed by the tool's output) -> the graph's nodes as an S1
    batch whose block c is column c (read_off, read_id, part), the paths' nodes [(column, row)] and ranges from the Q lines, the paths' reads and ranges from the P lines."""
    cols, q_nodes, q_ranges, p_reads, p_ranges = {}, [], [], [], []
    for ln in text.splitlines():
        x = ln.split("\t")
        if x[0] == "N":
            cols.setdefault(int(x[1]), []).extend((int(r), int(x[2])) for r in x[7:])
        elif x[0] == "Q":
            q_ranges.append((int(x[1]), int(x[2]))); q_nodes.append([tuple(int(v) for v in n.split(":")) for n in x[3:]])
        elif x[0] == "P":
            p_ranges.append((int(x[1]), int(x[2]))); p_reads.append(np.asarray([int(v) for v in x[3:]], np.uint32))
    n_cols = max(cols) + 1 if cols else 0
    read_off, read_id, part = [0], [], []
    for c in range(n_cols):
        for r, k in sorted(cols.get(c, [])):
            read_id.append(r); part.append(k)
        read_off.append(len(read_id))
    return (np.asarray(read_off, np.uint64), np.asarray(read_id, np.uint32), np.asarray(part, np.uint8)), q_nodes, q_ranges, p_reads, p_ranges


def join_stitch(text):
    """model(N lines, Q lines) and the P lines' lists, for comparison -> (model groups, Q ranges, P groups, P ranges)"""
    batch, q_nodes, q_ranges, p_reads, p_ranges = parse_stitch(text)
    return join(*batch, q_nodes), q_ranges, p_reads, p_ranges
