#!/usr/bin/env python3
"""Seeds of GSL's default generator (mt19937) whose fresh stream has an output word of 0 early on.  CPU only, numpy.

gsl_rng_uniform_pos skips such a word (probability 2^-32 per word), and a wavefront that draws the stream 64 pairs at a time
(csrc/mt_wave.h) redoes a chunk that holds one by a one-at-a-time walk.  A test of that walk needs a seed that has one; this
finds them.  The tempering is a bijection with temper(0) = 0, so an output word is 0 exactly where the state word is: the
search twists the state of many seeds at once and looks for zeros, it never tempers.

    python scripts/find_zero_word_seeds.py                       # seeds 1 .. 9 900 000, two states (1248 words) each
    python scripts/find_zero_word_seeds.py --first 7600000 --last 7630000

Searched: seeds 1 .. 9 900 000, the first two states of each (output words 0 .. 1247; 2.9 zeros expected), 240 to 300 s on
one core.  Two hits, both among the first 535 words (what a first block of 210 Gaussians consumes):

    seed 7603642   word 141 (counted from 0): the second word of its pair
    seed 7627928   word 400:                  the first word of its pair

They are the constants ZERO_WORD_SECOND and ZERO_WORD_FIRST of tests/hmc_stream.py, and tests/test_host_hmc_stream.py derives
both again with the oracle's generator.  The generator below is checked against numpy.random.RandomState (same algorithm,
same seeding) before the search starts."""
import argparse
import time

import numpy as np

N, M = 624, 397
U = np.uint32


def init_states(seeds):
    """gsl_rng_set / init_genrand for every seed: [624][len(seeds)] uint32 (seed 0 would be GSL's 4357)"""
    mt = np.empty((N, len(seeds)), dtype=U)
    prev = np.asarray(seeds, dtype=np.uint64)
    mt[0] = prev.astype(U)
    for i in range(1, N):
        prev = (np.uint64(1812433253) * (prev ^ (prev >> np.uint64(30))) + np.uint64(i)) & np.uint64(0xffffffff)
        mt[i] = prev.astype(U)
    return mt


def _step(mt, lo, hi, off):
    """mt[kk] for kk in [lo, hi) from mt[kk], mt[kk+1] and mt[kk+off]; the slices are chosen so that every word read is in the
    state the recurrence reads it in (old to the right, new to the left)"""
    y = (mt[lo:hi] & U(0x80000000)) | (mt[lo + 1:hi + 1] & U(0x7fffffff))
    mt[lo:hi] = mt[lo + off:hi + off] ^ (y >> U(1)) ^ np.where(y & U(1), U(0x9908b0df), U(0))


def twist(mt):
    """the next 624 words of every column, in place"""
    _step(mt, 0, N - M, M)                       # 0 .. 226 read old words only
    _step(mt, N - M, 2 * (N - M), M - N)         # 227 .. 453 read the new 0 .. 226
    _step(mt, 2 * (N - M), N - 1, M - N)         # 454 .. 622 read the new 227 .. 395
    y = (mt[N - 1] & U(0x80000000)) | (mt[0] & U(0x7fffffff))
    mt[N - 1] = mt[M - 1] ^ (y >> U(1)) ^ np.where(y & U(1), U(0x9908b0df), U(0))


def temper(k):
    k = k ^ (k >> U(11))
    k = k ^ ((k << U(7)) & U(0x9d2c5680))
    k = k ^ ((k << U(15)) & U(0xefc60000))
    return k ^ (k >> U(18))


def self_check():
    for seed in (1, 4357, 12345, 7603642, 0xFFFFFFFF):
        mt = init_states([seed])
        words = []
        for _ in range(2):
            twist(mt)
            words.append(temper(mt[:, 0].copy()))
        want = np.random.RandomState(seed).randint(0, 2 ** 32, size=2 * N, dtype=np.uint64).astype(U)
        assert np.array_equal(np.concatenate(words), want), seed


def search(first, last, states=2, batch=50000):
    hits = []
    for lo in range(first, last + 1, batch):
        seeds = np.arange(lo, min(lo + batch, last + 1), dtype=np.uint64)
        mt = init_states(seeds)
        for s in range(states):
            twist(mt)
            word, col = np.nonzero(mt == 0)
            hits += [(int(seeds[c]), s * N + int(w)) for w, c in zip(word, col)]
    return sorted(hits)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--first", type=int, default=1)
    ap.add_argument("--last", type=int, default=9900000)
    ap.add_argument("--states", type=int, default=2, help="states of 624 words searched per seed")
    a = ap.parse_args()
    self_check()
    t0 = time.time()
    found = search(a.first, a.last, a.states)
    for seed, word in found:
        print("seed %d: output word %d is 0 (%s word of a pair of a fresh stream without an earlier zero)" % (seed, word, "second" if word % 2 else "first"))
    print("%d seeds, %d words each, %.0f s: %d hits" % (a.last - a.first + 1, a.states * N, time.time() - t0, len(found)))
