"""Restatement of the optimise part of a call's launch plan (floria_hip.hip: plan_ploidies; optimize_kernel.h): which optimise instance every ploidy of a call takes.

The plan is made ONCE PER CALL from two numbers, the most reads of any block of the batch (n_max) and the widest SNP span of any block (span_max): the largest block
of the whole batch decides for every block, so a narrow block that is `HL` at every ploidy when it is phased alone loses the LDS histogram at the higher ploidies as
soon as a wide block of another contig rides in the same call (`call_shape`).  And the plan is made PER PLOIDY: the histogram of ploidy p takes span_max * p * A * 8
bytes, so one call can run the packed / delta instances at ploidy 2 and 3 and the generic HBM-histogram instance at 4 and 5 on the same block.

    hl      the job's histogram lives in LDS:  span_max*p*A*8 + span_max*p + 32 + moved_bytes + meta_bytes <= 60 KiB
    meta    (cell offset, length, partition | first, last) of every read staged in LDS, 12 bytes per read: n_max <= OPT_META_MAX (else meta_bytes = 0)
    opt_spec  the ploidy-specialised instances: biallelic, hl, 512 or 1024 threads, ploidy <= 5
    packed  ... reading the 4-byte cells ("opt_packed", every contig of the call uploaded with them): opt_spec at 512 threads
    delta   ... keeping integer distances and running delta passes ("opt_delta"): opt_spec at 512 threads with the metadata staged (and a span below 65 536)

The constants are the headers' documented values; tests/test_opt_limits_cpu.py checks the arithmetic against figures worked out by hand."""

LDS_BUDGET = 60 * 1024          # floria_hip.hip: plan_ploidies, the `hl` rule
META_BYTES_PER_READ = 12        # optimize_kernel.h: m_cb, m_lk, m_fl
OPT_META_MAX = 4096             # optimize_kernel.h
OPT_SORT_LDS = 512              # optimize_kernel.h: candidates sorted in LDS up to this many (M2, the power of two above the candidate count)
OPT_THREADS = 512               # the workgroup size of the instances that have a packed / delta form
MAX_SPEC_PLOIDY = 5


def moved_bytes(n_max):
    """the `moved` bitset: one bit per read, whole words, rounded up to 16 bytes"""
    return (((n_max + 31) // 32) * 4 + 15) & ~15


def meta_bytes(n_max):
    return ((n_max * META_BYTES_PER_READ + 15) & ~15) if n_max <= OPT_META_MAX else 0


def pow2_at_least(m):
    m2 = 1
    while m2 < m:
        m2 <<= 1
    return m2


def is_hl(n_max, span_max, alleles, p):
    return span_max * p * alleles * 8 + span_max * p + 32 + moved_bytes(n_max) + meta_bytes(n_max) <= LDS_BUDGET


def largest_hl_span(n_max, p, alleles=2):
    """the largest span_max for which ploidy p still keeps its histogram in LDS when the call's largest block has n_max reads (0 = none)"""
    room = LDS_BUDGET - 32 - moved_bytes(n_max) - meta_bytes(n_max)
    return max(0, room // (p * (alleles * 8 + 1)))


def smallest_non_hl_span(n_max, p, alleles=2):
    return largest_hl_span(n_max, p, alleles) + 1


def call_shape(blocks):
    """blocks: (reads, span) of EVERY non-empty block of the call, whatever contig it lies on -> (n_max, span_max), the two numbers the plan is made from"""
    blocks = list(blocks)
    return max([1] + [n for n, _ in blocks]), max([1] + [s for _, s in blocks])


def plan(n_max, span_max, alleles, P, opt_threads=OPT_THREADS, opt_packed=1, opt_delta=1, all_pk=True):
    """-> {p: {"hl", "meta", "opt_spec", "packed", "delta"}} for p = 1 .. P.  opt_threads: the forced workgroup size (128 | 512 | 1024; the library's own choice from
    the batch's mean reads per block is not restated here)."""
    assert opt_threads in (128, 512, 1024), opt_threads
    out = {}
    for p in range(1, P + 1):
        hl = is_hl(n_max, span_max, alleles, p)
        meta = n_max <= OPT_META_MAX
        spec = alleles == 2 and hl and opt_threads >= 512 and p <= MAX_SPEC_PLOIDY
        at512 = spec and opt_threads == OPT_THREADS
        out[p] = {"hl": hl, "meta": meta, "opt_spec": spec, "packed": bool(at512 and opt_packed and all_pk),
                  "delta": bool(at512 and opt_delta and meta and span_max <= 65535)}
    return out


def plan_for_blocks(blocks, alleles, P, **kw):
    """the plan of a call over these (reads, span) blocks: ONE plan, which every block of the call runs under"""
    n_max, span_max = call_shape(blocks)
    return plan(n_max, span_max, alleles, P, **kw)


def stages(P, fuse_p1=True):
    """the ploidies that have an optimise launch of their own in a call with one ploidy per stage and one job group: every ploidy up to P, whether or not a block is
    still open (the launches are queued without waiting for the stop rule), ploidy 1 left out where the ploidy-2 job stands for it ("fuse_p1", the default)"""
    return list(range(2 if (fuse_p1 and P >= 2) else 1, P + 1))


def launches(pl, P, fuse_p1=True):
    """-> (optimize_launches, optimize_packed_launches) of such a call"""
    st = stages(P, fuse_p1)
    return len(st), sum(1 for p in st if pl[p]["packed"])
