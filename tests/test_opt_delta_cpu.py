"""(no GPU) tests/opt_delta_model.py, the restatement of the optimise rounds that the "opt_delta" GPU test picks its inputs with: its cell search against
numpy's, and the whole model against the oracle (same optimised partition, same round count).  While it runs, the model itself asserts behind every accepted
round that exchanging the terms at the flipped code bytes gives the integers a full recomputation gives."""
import numpy as np

from tests import opt_delta_model as m
from tests.helpers import random_pileup

EPS = 0.03125


def test_find_cell_agrees_with_searchsorted_and_stays_inside_the_read():
    rng = np.random.default_rng(9100)
    shapes = [np.arange(1), np.arange(2), np.arange(300), np.arange(0, 600, 2), np.array([0, 1, 2, 50, 51, 52]), np.array([0, 299])]
    for _ in range(200):
        n = int(rng.integers(1, 120))
        gaps = (rng.random(n) < rng.choice([0.02, 0.2, 0.7])) * rng.integers(1, 9, size=n)
        gaps[0] = 0
        shapes.append(np.arange(n) + np.cumsum(gaps))
    worst = 0
    for deltas in shapes:
        for d in range(int(deltas[-1]) + 1):
            j, probes = m.find_cell(deltas, d)
            k = int(np.searchsorted(deltas, d))
            want = k if k < len(deltas) and int(deltas[k]) == d else -1
            assert j == want, (deltas, d, j, want)
            assert len(probes) <= 3 + int(np.ceil(np.log2(len(deltas) + 1))), (deltas, d, probes)
            worst = max(worst, len(probes))
    assert worst >= 3          # (the bisection steps were reached)
    dense = np.arange(300)
    assert all(len(m.find_cell(dense, d)[1]) == 1 for d in range(300)), "a dense read is found at the first guess"


def test_model_reproduces_the_oracle_and_the_update_is_exact(oracle_mod):
    w24 = oracle_mod.weight_q24()
    jobs = accepted = with_flips = 0
    for seed in range(9200, 9208):
        rng = np.random.default_rng(seed)
        n_snps = int(rng.integers(8, 49))
        pile = random_pileup(rng, int(rng.integers(8, 65)), n_snps, int(rng.integers(2, 5)), max_len=int(rng.integers(6, 25)), err=0.12, drop=float(rng.choice([0.0, 0.1, 0.4])))
        for ploidy in (2, 3, 4, 5):
            rid, pb, po, _, _, iters = oracle_mod.one_ploidy(pile, 1, n_snps, ploidy, EPS)
            if len(rid) == 0:
                continue
            part, it, rounds = m.run(pile, rid, pb, ploidy, EPS, w24)
            assert np.array_equal(part, po) and it == iters, (seed, ploidy, it, iters)
            jobs += 1
            for r in rounds:
                accepted += r["accepted"]
                with_flips += r["accepted"] and len(r["flips"]) > 0
    assert jobs >= 20 and accepted >= 12 and with_flips >= 6, (jobs, accepted, with_flips)
