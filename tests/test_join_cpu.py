"""No GPU: the numpy model of floria_hip_join_paths (tests/join_model.py) pinned to the C++ host — on the output of `floria-hip --stitch-graph FILE --stitch-paths`
(N lines: the nodes' reads, Q lines: every path's nodes, P lines: the reads the host's own union gives the path) the model of (N, Q) equals the P lines' lists, on
hand graphs and on 40 random layered graphs; the path peeling's two halves compose to what the tool printed before; the flags of the route are parsed."""
import subprocess

import numpy as np
import pytest

from tests import join_model as jm
from tests.test_host_cpu import floria_hip, random_graph  # noqa: F401  (the fixture builds the tool)


def stitch(tool, path, *extra):
    r = subprocess.run([tool, "--stitch-graph", path, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def check(tool, tmp_path, graph):
    path = str(tmp_path / "g.txt")
    open(path, "w").write(graph)
    plain = stitch(tool, path)
    out = stitch(tool, path, "--stitch-paths")
    assert [ln for ln in out.splitlines() if not ln.startswith("Q")] == plain.splitlines() and "Q\t" not in plain      # without the flag nothing changes
    model, q_ranges, p_reads, p_ranges = jm.join_stitch(graph + out)
    assert len(model) == len(p_reads) > 0 and q_ranges == p_ranges
    for k, (m, p) in enumerate(zip(model, p_reads)):
        assert np.array_equal(m, p), f"path {k}: {m} instead of {p}"
    return jm.parse_stitch(graph + out)


HAND = {
    # a chain of four one-row columns: one path through all of them, sink first
    "chain": "N\t0\t0\t0\t1\t1\t4\t0\t5\nN\t1\t0\t1\t1\t5\t8\t1\t5\nN\t2\t0\t2\t1\t9\t12\t2\t5\nN\t3\t0\t3\t1\t13\t16\t3\nE\t0\t0\t0\t7\nE\t1\t0\t0\t7\nE\t2\t0\t0\t7\n",
    # two rows a column, parallel chains that share reads 9 and 10 inside each chain (dedupe) and read 20 across the chains (a read in two groups)
    "two_chains": "N\t0\t0\t0\t1\t1\t4\t1\t9\t20\nN\t0\t1\t1\t1\t1\t4\t2\t10\t20\nN\t1\t0\t2\t1\t5\t8\t3\t9\nN\t1\t1\t3\t1\t5\t8\t4\t10\n"
                  "E\t0\t0\t0\t9\nE\t0\t1\t1\t9\n",
    # no edge at all: every node is a path of its own
    "no_edges": "N\t0\t0\t0\t1\t1\t4\t0\t1\nN\t0\t1\t1\t1\t1\t4\t2\nN\t1\t0\t2\t1\t5\t8\t1\t3\n",
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_graphs(floria_hip, tmp_path, name):
    batch, q_nodes, q_ranges, p_reads, _ = check(floria_hip, tmp_path, HAND[name])
    if name == "chain":
        assert q_nodes == [[(3, 0), (2, 0), (1, 0), (0, 0)]] and q_ranges == [(1, 16)] and p_reads[0].tolist() == [0, 1, 2, 3, 5]
    if name == "two_chains":
        assert sorted(map(sorted, q_nodes)) == [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]
        assert sorted(p.tolist() for p in p_reads) == [[1, 3, 9, 20], [2, 4, 10, 20]]
    if name == "no_edges":
        assert sorted(len(n) for n in q_nodes) == [1, 1, 1]


@pytest.mark.parametrize("seed", range(40))
def test_random_layered_graphs(floria_hip, tmp_path, seed):
    rng = np.random.default_rng(700 + seed)
    batch, q_nodes, _, _, _ = check(floria_hip, tmp_path, random_graph(rng, int(rng.integers(2, 12)), int(rng.integers(1, 5))))
    read_off, read_id, part = batch
    n_nodes = sum(len(set(part[int(read_off[c]):int(read_off[c + 1])].tolist())) for c in range(len(read_off) - 1))
    assert sorted(n for p in q_nodes for n in p) == sorted(set(n for p in q_nodes for n in p)) and sum(len(p) for p in q_nodes) == n_nodes      # every node on exactly one path


def test_the_route_flag_is_parsed(floria_hip, tmp_path):
    r = subprocess.run([floria_hip, "-b", "x.bam", "-v", "x.vcf", "-r", "x.fa", "-o", str(tmp_path / "o"), "--paths", "bogus"], capture_output=True, text=True)
    assert r.returncode != 0 and "--paths takes host or resident, not 'bogus'" in r.stderr
    r = subprocess.run([floria_hip, "--help"], capture_output=True, text=True)
    assert "--paths host|resident" in r.stderr and "floria_hip_join_paths" in r.stderr
