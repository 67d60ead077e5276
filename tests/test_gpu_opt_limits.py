"""(GPU) the optimise kernel's packed ("opt_packed") and delta ("opt_delta") instances at their size limits (optimize_kernel.h; floria_hip.hip: plan_ploidies):
more reads in a block than the workgroup has threads, candidate lists on both sides of the LDS sort (OPT_SORT_LDS), the LDS budget that decides per ploidy and per
call whether the histogram lives in LDS (`HL`: only then is there a packed or a delta instance), and the reads per block up to which the metadata is staged
(OPT_META_MAX).

Every case is one call (or two) with speculate = 0, opt_threads = 512 and one job group, so that a ploidy stage is one optimise launch: optimize_launches is then the
number of stages (ploidies 2 .. P, ploidy 1 rides in the ploidy-2 job) whether or not a block is still open, and optimize_packed_launches the number of those whose
plan is `HL`.  The call runs under the default options, under opt_packed = 0 and under opt_delta = 0: the three results are equal bit for bit (best_ploidy,
ploidies_tried, mec as uint64, read_off, read_id, part, min_prune_margin) and equal to the oracle's, and the counters are what tests/opt_plan_model.py (launches) and
tests/opt_delta_model.py (delta passes, fallbacks: exact, every job of the call restated) say.  The inputs come from tests/opt_limits_cases.py;
tests/test_opt_limits_cpu.py asserts on the CPU that each is what its name says, the cheap part of which is repeated here before the call.  Every test prints its
counters beside the prediction."""
import numpy as np
import pytest

from tests import opt_limits_cases as cases
from tests import opt_plan_model as pm
from tests.test_gpu_opt_delta import knobs          # noqa: F401  (the fixture: sets options, puts the defaults back)
from tests.test_gpu_opt_packed import Case, same_bits

pytestmark = pytest.mark.gpu

CONFIGS = [("default", {}), ("opt_packed=0", {"opt_packed": 0}), ("opt_delta=0", {"opt_delta": 0})]


def flags(pl, key):
    return {p for p, v in pl.items() if v[key]}


def three_ways(ctx, lib, oracle, spec, set_knobs, pre=None):
    """the call under the three option sets: results equal to each other and to the oracle, counters as the models predict; pre(tried, accounts): the case's precondition
    on the ploidies the reference tries and on the model's account of every block (cases.account), asserted before the first call; -> the result under the defaults"""
    case = Case(oracle, spec.pileups, spec.blocks(), P=spec.P)
    n_contigs = len(spec.pileups)
    assert [int(np.diff(case.oracle[i].read_off.astype(np.int64))[0]) for i in range(n_contigs)] == [n for n, _ in spec.shapes()], "a block does not hold every read"
    tried = [int(case.oracle[i].ploidies_tried[0]) for i in range(n_contigs)]
    passes, fallbacks, acc = cases.predict(oracle, spec, tried, spec.plan())          # (opt_packed = 0 has the same pass on the 8-byte cells; opt_delta = 0 has none)
    if pre is not None:
        pre(tried, acc)
    res = ctx.upload_batch(spec.pileups)
    out, counters = [], []
    try:
        set_knobs(speculate=0, opt_threads=512, groups=1)
        for name, kv in CONFIGS:
            set_knobs(opt_packed=1, opt_delta=1)
            set_knobs(**kv)
            pl = spec.plan(opt_packed=kv.get("opt_packed", 1), opt_delta=kv.get("opt_delta", 1))
            launches, packed = pm.launches(pl, spec.P)
            want = (passes, fallbacks) if kv.get("opt_delta", 1) else (0, 0)
            assert flags(pl, "delta") == (flags(spec.plan(), "delta") if kv.get("opt_delta", 1) else set())
            r = ctx.phase_blocks_batch(res, case.bc, case.bs, case.be, lib.make_params(cases.EPS, spec.P, 10))
            t = ctx.timing()
            print(f"{spec.name} [{name}]: optimize_launches {t['optimize_launches']} (predicted {launches}), optimize_packed_launches {t['optimize_packed_launches']} "
                  f"(predicted {packed}), optimize_delta_passes {t['optimize_delta_passes']} (predicted {want[0]}), optimize_delta_fallbacks "
                  f"{t['optimize_delta_fallbacks']} (predicted {want[1]}); ploidies tried {tried}")
            counters.append((name, (t["optimize_launches"], t["optimize_packed_launches"]), (launches, packed), (t["optimize_delta_passes"], t["optimize_delta_fallbacks"]), want))
            out.append(r)
    finally:
        for x in res:
            x.free()
    # the results first: a call that took another instance than the plan model says must still compute the same bits, and the failure says which of the two went wrong
    for (name, _), r in zip(CONFIGS[1:], out[1:]):
        same_bits(out[0], r, f"{spec.name}: {name} against the default")
    for (name, _), r in zip(CONFIGS, out):
        case.check_oracle(r, f"{spec.name}: {name}")
    for name, got_l, want_l, got_d, want_d in counters:
        assert got_l == want_l, f"{spec.name} [{name}]: (optimize_launches, optimize_packed_launches) {got_l}, the plan model says {want_l}"
        assert got_d == want_d, f"{spec.name} [{name}]: (optimize_delta_passes, optimize_delta_fallbacks) {got_d}, the delta model says {want_d}"
    return out[0]


def test_a_reads_per_block_around_512_and_1024(gpu_ctx, hip_lib, oracle_mod, knobs):
    """One block each of 511, 512, 513, 1 023, 1 025 reads: the per-read loops of the kernel (metadata staging, bucket scatter, the reduction that decides the pass, the delta
    pass itself) take a second and a third trip.  First the blocks of up to 513 reads in a call of their own, then all five in one batch; the model restates every job
    of both calls (two seconds on the CPU), so the delta counters are exact in both.  The three larger blocks are seeded so that a delta pass which stopped at read 512
    would change a partition (tests/test_opt_limits_cpu.py)."""
    spec = cases.case_a()
    assert [n for n, _ in spec.shapes()] == cases.A_COUNTS
    small = spec.sub("a: 511 / 512 / 513 reads, a call of their own", [0, 1, 2])

    def late_reads_meet_flips(tried, acc):
        for a in acc:
            assert len(a["reads"]) <= 512 or (a["passes"] >= 1 and cases.flip_reaches_read_from(a, 512)), len(a["reads"])

    for s in (small, spec):
        assert flags(s.plan(), "packed") == flags(s.plan(), "delta") == {1, 2, 3, 4, 5}
        three_ways(gpu_ctx, hip_lib, oracle_mod, s, knobs, pre=late_reads_meet_flips)


def test_b_candidate_lists_on_both_sides_of_the_lds_sort(gpu_ctx, hip_lib, oracle_mod, knobs):
    """Two constructed blocks of 331 / 332 reads (tests/opt_limits_cases.py says how and why not seeded ones: no seeded search came near 512 candidates): at ploidy 4
    round 0 has 735 / 738 candidates — sorted in the global pools — flips one code byte and is accepted, so round 1 opens with a delta pass whose flip list was written
    into s_key behind a pool sort; round 1 has 510 / 513 candidates, two short of a full LDS sort and one past it."""
    spec = cases.case_b()
    assert flags(spec.plan(), "packed") == flags(spec.plan(), "delta") == {1, 2, 3, 4, 5}

    def rounds_around_the_lds_sort(tried, acc):
        for a in acc:
            rounds = a["rounds"][4]
            assert rounds[0]["M2"] > pm.OPT_SORT_LDS and rounds[0]["accepted"] and rounds[0]["pass"] == "delta" and rounds[1]["accepted"]
        assert [a["rounds"][4][1]["M"] for a in acc] == [510, 513]

    three_ways(gpu_ctx, hip_lib, oracle_mod, spec, knobs, pre=rounds_around_the_lds_sort)


@pytest.mark.parametrize("extra", [0, 1])
def test_c_the_hl_edge_at_ploidy_3(gpu_ctx, hip_lib, oracle_mod, knobs, extra):
    """100 reads of 20-60 cells over the largest span whose ploidy-3 histogram still fits LDS (1 180 with 100 reads: computed, not written down) and over one SNP more.
    At the first span the dynamic LDS request of the ploidy-3 launch is at its maximum beside the kernel's static arrays; ploidies 2 and 3 take packed launches and
    integer distances, 4 and 5 the HBM-histogram instance, seeded by the partition of the ploidy below.  The launches per stage are derivable — every stage is queued,
    one job group, ploidy 1 fused — so the counters are asserted exactly: 4 optimise launches, 2 packed (1 at span + 1), and the model's delta counters over the HL
    ploidies only."""
    spec = cases.case_c(extra)
    span = pm.largest_hl_span(cases.C_READS, 3) + extra
    assert spec.shapes() == [(cases.C_READS, span)]
    pl = spec.plan()
    assert flags(pl, "packed") == flags(pl, "delta") == ({1, 2, 3} if extra == 0 else {1, 2})
    launches, packed = pm.launches(pl, spec.P)
    assert 0 < packed < launches and packed == len([p for p in pm.stages(spec.P) if pl[p]["hl"]])

    def reaches_ploidy_4(tried, acc):
        assert tried[0] >= 4 and sorted(acc[0]["rounds"]) == ([2, 3] if extra == 0 else [2])

    three_ways(gpu_ctx, hip_lib, oracle_mod, spec, knobs, pre=reaches_ploidy_4)


def test_d_the_largest_block_of_the_batch_decides_for_every_block(gpu_ctx, hip_lib, oracle_mod, knobs):
    """A 60-SNP block of 100 reads, alone — packed at every ploidy — and in a batch with a second contig whose block has the largest span that is HL at ploidy 2: now it is
    packed at ploidy 2 only, and gives the same bits."""
    alone, batch = cases.case_d(False), cases.case_d(True)
    assert pm.launches(alone.plan(), 5) == (4, 4) and pm.launches(batch.plan(), 5) == (4, 1)
    ra = three_ways(gpu_ctx, hip_lib, oracle_mod, alone, knobs)
    rb = three_ways(gpu_ctx, hip_lib, oracle_mod, batch, knobs)
    n = int(ra.read_off[1])
    assert int(ra.best_ploidy[0]) == int(rb.best_ploidy[0]) and np.array_equal(ra.mec[0].view(np.uint64), rb.mec[0].view(np.uint64))
    assert int(rb.read_off[1]) == n and np.array_equal(ra.part[:n], rb.part[:n]) and np.array_equal(ra.read_id[:n], rb.read_id[:n])


@pytest.mark.parametrize("n_reads", [4096, 4097])
def test_e_reads_per_block_at_opt_meta_max(gpu_ctx, hip_lib, oracle_mod, knobs, n_reads):
    """4 096 reads: the staged metadata takes 48 KiB, the 300-SNP block is HL (packed, delta) at ploidy 2 only.  4 097 reads: nothing is staged, every ploidy is HL and
    packed — the packed instance reads its metadata from HBM and has no visiting order — and no job keeps integer distances: both delta counters stay 0."""
    spec = cases.case_e(n_reads)
    assert spec.shapes() == [(n_reads, cases.E_SNPS)]
    pl = spec.plan()
    if n_reads <= pm.OPT_META_MAX:
        assert flags(pl, "packed") == flags(pl, "delta") == {1, 2}
    else:
        assert flags(pl, "packed") == {1, 2, 3, 4, 5} and not flags(pl, "delta")

    def beyond_ploidy_2(tried, acc):
        assert tried[0] >= 3 and (acc[0]["passes"] >= 1) == (n_reads <= pm.OPT_META_MAX)

    three_ways(gpu_ctx, hip_lib, oracle_mod, spec, knobs, pre=beyond_ploidy_2)


def test_f_four_alleles_at_513_reads(gpu_ctx, hip_lib, oracle_mod, knobs):
    """alleles 0-3: the generic instances, neither packed nor delta, whatever the options say"""
    spec = cases.case_f()
    assert spec.shapes() == [(513, cases.NARROW)] and set(int(x) for x in spec.pileups[0].allele) == {0, 1, 2, 3}
    assert pm.launches(spec.plan(), 5) == (4, 0) and not flags(spec.plan(), "delta")
    three_ways(gpu_ctx, hip_lib, oracle_mod, spec, knobs)
