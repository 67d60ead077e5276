"""`-m gpu`: S1 and the kernels behind it at SNP indices past 65 536, with reads of up to 10 001 cells and blocks of up to 65 536 positions (the worlds of
tests/wide_cases.py; tests/test_wide_cases_cpu.py pins their shapes).  Until this file every S1 / S2 test placed its SNPs at 1 .. 50 000, in blocks of at most
2 600 positions and reads of at most ~1 500 cells.

Every expectation is the oracle on the same, moved input, bit for bit (assert_block_results_equal and min_prune_margin ==); in the canonical arithmetic the
result must also equal the device's own on the unmoved world.
  (a) every beam kernel, sequential and speculative stages, the general insert path: the state hash across its wrap at 65 536 and far past it;
  (b) the same worlds in the reference arithmetic, whose emulated hash containers are keyed by the absolute SNP index;
  (c) one batch holding the same contig in three coordinate systems, through the three upload routes;
  (d) reads on both sides of 4 096 cells up to the longest a block takes, and the one SNP longer that it must leave out;
  (e) a block of exactly 65 536 positions, and the refusal of 65 537;
  (f) hap_graph, S2 and the haploset consumers on the batch of (c).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from floria_amd import _capi as capi
from tests import wide_cases as wc
from tests.helpers import assert_block_results_equal

pytestmark = pytest.mark.gpu
EPS = 0.03125
NON_DYADIC = (0.04, 0.05, 0.0437)
KNOB_RESET = (("beam_path", 0), ("speculate", -1), ("no_bulk", 0), ("no_specialized", 0), ("arith_replay", 0), ("arith_hbm", 0), ("upload_chunks", 0))


@pytest.fixture()
def arith(gpu_ctx, oracle_mod):
    gpu_ctx.set_option("arith", 1)
    oracle_mod.set_arith_mode(1)
    yield gpu_ctx
    oracle_mod.set_arith_mode(0)
    gpu_ctx.set_option("arith", 0)


@pytest.fixture()
def knobs(gpu_ctx):
    """set_option for the test; every knob this file touches is back at its default afterwards, whatever happened"""
    try:
        yield gpu_ctx.set_option
    finally:
        for k, v in KNOB_RESET:
            gpu_ctx.set_option(k, v)


def same(want, got, what):
    assert_block_results_equal(want, got, what)
    assert want.min_prune_margin == got.min_prune_margin, what


def on_oracle(oracle_mod, w, eps):
    return oracle_mod.phase_blocks(w.pile, w.s, w.e, oracle_mod.make_params(eps, w.P, w.B), threads=8)


def on_device(ctx, hip_lib, contig, w, eps):
    return ctx.phase_blocks(contig, w.s, w.e, hip_lib.make_params(eps, w.P, w.B))


def world_of(kind, seed):
    return wc.dup_world(seed) if kind == "dup" else wc.medium_world(seed)


# ---- (a) the state hash across its wrap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", ["dup", "medium"])
def test_every_beam_kernel_at_wrap_and_far_indices(gpu_ctx, hip_lib, oracle_mod, knobs, kind, seed):
    """hash_idx() wraps the absolute SNP index at 65 536; the slab and wide kernels form their window-exit terms from pos0 + offset, the flatten kernel the
    reads' constants from the cells' SNPs.  Were one site to disagree with another past the wrap, equal states would stop being recognised as duplicates - on
    the cloned reads of dup_world in almost every step."""
    w0 = world_of(kind, seed)
    eps = (EPS, 0.04)[seed % 2]
    home = on_device(gpu_ctx, hip_lib, w0.pile, w0, eps)
    same(on_oracle(oracle_mod, w0, eps), home, f"{kind} {seed} unmoved")
    for name, k in wc.offsets(w0).items():
        w = wc.shifted(w0, k)
        ro = on_oracle(oracle_mod, w, eps)
        rc = gpu_ctx.upload(w.pile)
        try:
            runs = [(("beam_path", path), ("speculate", spec)) for path in (2, 1, 3) for spec in (0, 1)]
            if kind == "dup":
                runs += [(("no_bulk", 1), ("speculate", spec)) for spec in (0, 1)] + [(("no_bulk", 0), ("speculate", -1))]
            runs += [(("no_specialized", 1),)]
            for run in runs:
                for key, v in KNOB_RESET:
                    knobs(key, v)
                for key, v in run:
                    knobs(key, v)
                rg = on_device(gpu_ctx, hip_lib, rc, w, eps)
                same(ro, rg, f"{kind} {seed} at {name} ({k}) {run}")
                same(home, rg, f"{kind} {seed} at {name} ({k}) {run} against the unmoved world")
        finally:
            rc.free()


# ---- (b) the reference arithmetic --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", ["dup", "medium"])
def test_reference_arithmetic_at_wrap_and_far_indices(arith, hip_lib, oracle_mod, knobs, kind, seed):
    """The emulated FxHashSet / FxHashMap orders (cell_order_direct_kernel's home-bucket rule, cell_order_kernel, the position maps of optimize_kernel.h) are
    functions of the absolute positions: a moved pileup is a new input (tests/test_wide_cases_cpu.py), and no key >= 65 536 had been through them on the device."""
    w0 = world_of(kind, seed)
    eps = NON_DYADIC[seed % 3]
    for name, k in [("home", 0)] + list(wc.offsets(w0).items()):
        w = wc.shifted(w0, k)
        ro = on_oracle(oracle_mod, w, eps)
        rc = arith.upload(w.pile)
        try:
            same(ro, on_device(arith, hip_lib, rc, w, eps), f"{kind} {seed} at {name} ({k}) eps {eps}")
            if name == "far":
                for knob in ("arith_replay", "arith_hbm"):
                    knobs(knob, 1)
                    same(ro, on_device(arith, hip_lib, rc, w, eps), f"{kind} {seed} at far, {knob}")
                    knobs(knob, 0)
        finally:
            rc.free()


# ---- (c) one batch, three coordinate systems ----------------------------------------------------------------------------------------------------------------------
BATCH_WORLDS = {"dup1": lambda: wc.dup_world(1), "medium1_q0": lambda: wc.medium_world(1), "medium2_four_alleles": lambda: wc.medium_world(2)}


@functools.lru_cache(maxsize=None)
def batch_of(which):
    """the same world unmoved, at K_WRAP and at K_FAR as contigs 0, 1, 2 of one call -> (offsets, worlds, blk_contig, blk_start, blk_end)"""
    w0 = BATCH_WORLDS[which]()
    ks = (0, wc.k_wrap(w0), wc.K_FAR)
    ws = [wc.shifted(w0, k) for k in ks]
    bc = np.repeat(np.arange(3, dtype=np.uint32), len(w0.s))
    return ks, ws, bc, np.concatenate([w.s for w in ws]), np.concatenate([w.e for w in ws])


def blocks_of(r, b0, b1):
    """blocks [b0, b1) of a batch result, as a result of their own"""
    lo, hi = int(r.read_off[b0]), int(r.read_off[b1])
    return SimpleNamespace(best_ploidy=r.best_ploidy[b0:b1], ploidies_tried=r.ploidies_tried[b0:b1], read_off=r.read_off[b0:b1 + 1] - r.read_off[b0],
                           read_id=r.read_id[lo:hi], part=r.part[lo:hi], mec=np.ascontiguousarray(r.mec[b0:b1]))


def check_batch(r, ros, alone, what):
    nb = ros[0].n_blocks
    assert r.n_blocks == 3 * nb
    for i in range(3):
        got = blocks_of(r, i * nb, (i + 1) * nb)
        assert_block_results_equal(ros[i], got, f"{what}: contig {i} against the oracle")
        assert_block_results_equal(alone[i], got, f"{what}: contig {i} against the contig phased alone")
    assert r.min_prune_margin == min(x.min_prune_margin for x in ros), what


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("which", sorted(BATCH_WORLDS))
def test_one_batch_three_coordinate_systems(gpu_ctx, hip_lib, oracle_mod, knobs, which, mode):
    ks, ws, bc, bs, be = batch_of(which)
    piles = [w.pile for w in ws]
    eps = 0.04
    par = hip_lib.make_params(eps, ws[0].P, ws[0].B)
    gpu_ctx.set_option("arith", mode); oracle_mod.set_arith_mode(mode)
    try:
        ros = [on_oracle(oracle_mod, w, eps) for w in ws]
        alone = [on_device(gpu_ctx, hip_lib, w.pile, w, eps) for w in ws]
        for i in range(3):
            same(ros[i], alone[i], f"{which} mode {mode}: contig {i} alone")
            if mode == 0:
                same(alone[0], alone[i], f"{which}: contig {i} alone against the unmoved contig")
        hs = gpu_ctx.upload_batch(piles)
        try:
            check_batch(gpu_ctx.phase_blocks_batch(hs, bc, bs, be, par), ros, alone, f"{which} mode {mode} upload_batch")
        finally:
            for h in hs:
                h.free()
        arena, parr, _ = hip_lib.pack_pileups(piles)
        try:
            cb = gpu_ctx.upload_batch_packed(parr)
            try:
                check_batch(gpu_ctx.phase_blocks_batch(cb, bc, bs, be, par), ros, alone, f"{which} mode {mode} upload_batch_packed")
            finally:
                cb.free()
        finally:
            arena.free()
        arena, pinned = hip_lib.pin_pileups(piles)
        try:
            knobs("upload_chunks", 2)
            r = gpu_ctx.phase_pileups_batch(pinned, bc, bs, be, par)
            assert gpu_ctx.timing()["upload_chunks"] == 2
            check_batch(r, ros, alone, f"{which} mode {mode} phase_pileups_batch in 2 chunks")
        finally:
            arena.free()
    finally:
        gpu_ctx.set_option("arith", 0); oracle_mod.set_arith_mode(0)


# ---- (d) long reads ---------------------------------------------------------------------------------------------------------------------------------------------------
LONG_K = 65536 - 6000


def check_long_blocks(w, r):
    span = w.pile.last.astype(np.int64) - w.pile.first + 1
    for b in range(r.n_blocks):
        ids = r.block(b)[0]
        assert len(ids) == 30 and not np.isin(np.nonzero(span == 10002)[0], ids).any() and np.isin(np.nonzero(span == 10001)[0], ids).all()


@pytest.mark.parametrize("mode", (0, 1))
def test_reads_of_4095_to_10001_cells(gpu_ctx, hip_lib, oracle_mod, knobs, mode):
    """Reads of 4 095 / 4 096 / 4 097 cells (from 4 096 on the first-insertion keys of the reference arithmetic no longer fit `read << 12 | cell rank`; more than
    1 792 cells leave cell_order_direct_kernel's table), of 10 001 (the longest a block takes: 40 LDS tiles in the beam kernels) and of 10 002, which every block
    must leave out; unmoved and with index 65 536 inside both blocks; the default beam kernel and the generic one."""
    w0 = wc.long_world()
    assert int(np.diff(w0.pile.read_off).max()) >= 4096                                       # len_max, what the context's switch looks at
    eps = 0.04
    gpu_ctx.set_option("arith", mode); oracle_mod.set_arith_mode(mode)
    try:
        home = None
        for k in (0, LONG_K):
            w = wc.shifted(w0, k)
            ro = on_oracle(oracle_mod, w, eps)
            check_long_blocks(w, ro)
            rc = gpu_ctx.upload(w.pile)
            try:
                for path in (0, 1):
                    knobs("beam_path", path)
                    rg = on_device(gpu_ctx, hip_lib, rc, w, eps)
                    same(ro, rg, f"mode {mode} offset {k} beam_path {path}")
                    check_long_blocks(w, rg)
                    home = home or rg
                    if mode == 0:
                        same(home, rg, f"offset {k} beam_path {path} against the unmoved world")
                knobs("beam_path", 0)
            finally:
                rc.free()
    finally:
        gpu_ctx.set_option("arith", 0); oracle_mod.set_arith_mode(0)


def test_long_reads_on_a_context_that_has_only_seen_short_ones(hip_lib, oracle_mod):
    """The switch between 32-bit and 64-bit first-insertion keys is a property of the call in flight, kept on the context: a context whose first call held reads
    of a dozen cells must give the long world the same bits."""
    short, w = wc.dup_world(0), wc.shifted(wc.long_world(), LONG_K)
    eps = 0.04
    ctx = hip_lib.FloriaHip(0)
    oracle_mod.set_arith_mode(1)
    try:
        ctx.set_option("arith", 1)
        same(on_oracle(oracle_mod, short, eps), on_device(ctx, hip_lib, short.pile, short, eps), "the short-read contig")
        ro = on_oracle(oracle_mod, w, eps)
        same(ro, on_device(ctx, hip_lib, w.pile, w, eps), "the long world behind it")
        same(on_oracle(oracle_mod, short, eps), on_device(ctx, hip_lib, short.pile, short, eps), "and short reads again")
    finally:
        oracle_mod.set_arith_mode(0)
        ctx.close()


# ---- (e) the span limit ---------------------------------------------------------------------------------------------------------------------------------------------
limit_world = functools.lru_cache(maxsize=None)(wc.span_limit_world)


@pytest.mark.parametrize("mode", (0, 1))
def test_a_block_of_exactly_65536_positions(gpu_ctx, hip_lib, oracle_mod, knobs, mode):
    """span == HASH_M: the state hash's window is as long as its period, the optimise kernel's histogram and position maps lie in HBM, the incremental distance
    pass sits on its `span <= 65535` guard; unmoved and at K_FAR (where the window wraps inside the block)."""
    w0 = limit_world(0)
    eps = 0.04
    gpu_ctx.set_option("arith", mode); oracle_mod.set_arith_mode(mode)
    try:
        home = None
        for k in (0, wc.K_FAR):
            w = wc.shifted(w0, k)
            ro = on_oracle(oracle_mod, w, eps)
            assert int(ro.best_ploidy[0]) == 2 and len(ro.block(0)[0]) == 900
            rc = gpu_ctx.upload(w.pile)
            try:
                for path in (0, 1):
                    knobs("beam_path", path)
                    rg = on_device(gpu_ctx, hip_lib, rc, w, eps)
                    same(ro, rg, f"mode {mode} offset {k} beam_path {path}")
                    home = home or rg
                    if mode == 0:
                        same(home, rg, f"offset {k} beam_path {path} against the unmoved world")
                knobs("beam_path", 0)
            finally:
                rc.free()
    finally:
        gpu_ctx.set_option("arith", 0); oracle_mod.set_arith_mode(0)


def test_a_block_of_65536_positions_with_four_alleles(gpu_ctx, hip_lib, oracle_mod):
    """... where span * alleles is exactly the length of the hash multiplier tables (4 * HASH_M)"""
    w = limit_world(0, 4)
    assert int(w.pile.allele.max()) == 3
    same(on_oracle(oracle_mod, w, 0.04), on_device(gpu_ctx, hip_lib, w.pile, w, 0.04), "four alleles")


def test_a_block_of_65537_positions_is_refused_and_the_context_lives_on(gpu_ctx, hip_lib, oracle_mod):
    w0, w1 = limit_world(0), limit_world(1)
    first = on_device(gpu_ctx, hip_lib, w0.pile, w0, 0.04)
    with pytest.raises(hip_lib.FloriaHipError, match="a block's reads span more than 65536 SNPs") as ei:
        on_device(gpu_ctx, hip_lib, w1.pile, w1, 0.04)
    assert ei.value.code == capi.FLORIA_E_UNSUPPORTED
    again = on_device(gpu_ctx, hip_lib, w0.pile, w0, 0.04)
    same(first, again, "after the refusal")
    same(on_oracle(oracle_mod, w0, 0.04), again, "after the refusal, against the oracle")


# ---- (f) after S1 -------------------------------------------------------------------------------------------------------------------------------------------------------
def f64_same(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("which", sorted(BATCH_WORLDS))
def test_graph_s2_and_haploset_consumers_on_the_three_coordinate_systems(gpu_ctx, hip_lib, oracle_mod, which, mode):
    from tests.test_gpu_parity import groups_from_blocks
    ks, ws, bc, bs, be = batch_of(which)
    piles = [w.pile for w in ws]
    nb = len(ws[0].s)
    eps = 0.04
    gpu_ctx.set_option("arith", mode); oracle_mod.set_arith_mode(mode)
    hs = gpu_ctx.upload_batch(piles)
    sets = None
    try:
        # hap_graph on the batch that is still resident
        r = gpu_ctx.phase_blocks_batch(hs, bc, bs, be, hip_lib.make_params(eps, ws[0].P, ws[0].B))
        g = gpu_ctx.hap_graph(r)
        assert np.array_equal(np.diff(g.node_off), r.best_ploidy)
        per = []
        for i, w in enumerate(ws):
            ro = on_oracle(oracle_mod, w, eps)
            cov, ew = oracle_mod.hap_graph(w.pile, w.s, w.e, ro)
            lo, hi = int(g.node_off[i * nb]), int(g.node_off[(i + 1) * nb])
            assert np.array_equal(cov.view(np.uint64), g.node_cov[lo:hi].view(np.uint64)), f"contig {i} node coverage"
            elo, ehi = int(g.edge_off[i * nb]), int(g.edge_off[(i + 1) * nb])
            assert np.array_equal(ew, g.edge_w[elo:ehi]), f"contig {i} edge weights"
            assert g.pred[i * nb] == -1
            per.append(groups_from_blocks(blocks_view(r, i * nb, (i + 1) * nb), w.s, w.e))
        assert g.edge_w.sum() > 0
        # S2 with groups taken from the S1 partitions: by arrays, and resident
        gc, groups, ranges = [], [], []
        for i, (gr, rg) in enumerate(per):
            gc += [i] * len(gr); groups += gr; ranges += rg
        out = gpu_ctx.reassign_batch(hs, gc, groups, ranges, eps)
        sets = gpu_ctx.reassign_batch_resident(hs, gc, groups, ranges, eps)
        down = sets.download()
        for i, w in enumerate(ws):
            go = oracle_mod.reassign(w.pile, per[i][0], per[i][1], eps)
            for got, what in ((out[i], "reassign_batch"), (down[i], "reassign_batch_resident")):
                assert go.n_groups == got.n_groups, f"{what} contig {i}"
                assert np.array_equal(go.range, got.range) and np.array_equal(go.grp_off, got.grp_off) and np.array_equal(go.grp_read, got.grp_read), f"{what} contig {i}"
            if mode == 0:
                assert np.array_equal(out[i].grp_off, out[0].grp_off) and np.array_equal(out[i].grp_read, out[0].grp_read), f"contig {i} against the unmoved contig"
                assert np.array_equal(out[i].range.astype(np.int64), out[0].range.astype(np.int64) + ks[i]), f"contig {i}: ranges + {ks[i]}"
        assert sum(x.n_groups for x in out) > 0
        # the consumers, on the haplosets S2 returned: by arrays and by handle
        hc, hgroups, hranges = [], [], []
        for i, x in enumerate(out):
            for k in range(x.n_groups):
                hc.append(i); hgroups.append(x.group(k)); hranges.append(tuple(int(v) for v in x.range[k]))
        st = gpu_ctx.haploset_stats(hs, hc, hgroups, hranges)
        st_h = gpu_ctx.haploset_stats(hs, haplosets=sets)
        assert f64_same(st, st_h)
        for k in range(len(hgroups)):
            assert f64_same(oracle_mod.haploset_stats(piles[hc[k]], hgroups[k], hranges[k][0], hranges[k][1]), st[k]), f"haploset {k} of contig {hc[k]}"
        pos_off, counts = gpu_ctx.haploset_alleles(hs, hc, hgroups, hranges)
        pos_h, counts_h = gpu_ctx.haploset_alleles(hs, haplosets=sets)
        assert np.array_equal(pos_off, pos_h) and np.array_equal(counts, counts_h)
        want = np.zeros_like(counts)
        for k, (grp, (lo, hi)) in enumerate(zip(hgroups, hranges)):
            p = piles[hc[k]]
            for rd in grp:
                s, a, _ = p.read(int(rd))
                m = (s >= lo) & (s <= hi)
                np.add.at(want, (int(pos_off[k]) + (s[m].astype(np.int64) - lo), a[m].astype(np.int64)), 1)
        assert np.array_equal(counts, want) and counts.any()
        # genome positions for every SNP index up to the contig's last: a dummy ramp below the offset, the same steps behind it in every coordinate system
        steps = np.cumsum(np.random.default_rng(5).integers(50, 400, size=ws[0].S + 1)).astype(np.uint64)
        pos = [np.concatenate([np.arange(1, k + 1, dtype=np.uint64), np.uint64(k + 1000) + steps]) for k in ks]
        assert all(len(p) > int(w.pile.last.max()) for p, w in zip(pos, ws))
        hq, rel, avg = gpu_ctx.hapq_batch(hs, hc, hgroups, hranges, pos, 2000)
        hq_h, rel_h, avg_h = gpu_ctx.hapq_batch(hs, snp_positions=pos, block_length=2000, haplosets=sets)
        assert np.array_equal(hq, hq_h) and f64_same(rel, rel_h) and f64_same(avg, avg_h)
        o = 0
        for i in range(3):
            n = out[i].n_groups
            ohq, orel, oavg = oracle_mod.hapq(piles[i], hgroups[o:o + n], hranges[o:o + n], pos[i], 2000)
            assert np.array_equal(hq[o:o + n], ohq), f"contig {i} hapq"
            assert f64_same(rel[o:o + n], orel) and f64_same([avg[i]], [oavg]), f"contig {i} rel_err / avg_err"
            o += n
    finally:
        if sets is not None:
            sets.free()
        for h in hs:
            h.free()
        gpu_ctx.set_option("arith", 0); oracle_mod.set_arith_mode(0)


def blocks_view(r, b0, b1):
    """blocks [b0, b1) of a batch result with the two accessors groups_from_blocks uses"""
    v = blocks_of(r, b0, b1)
    v.n_blocks = b1 - b0
    v.block = lambda b: (v.read_id[int(v.read_off[b]):int(v.read_off[b + 1])], v.part[int(v.read_off[b]):int(v.read_off[b + 1])])
    v.partitions = lambda b: [v.block(b)[0][v.block(b)[1] == k] for k in range(int(v.best_ploidy[b]))]
    return v
