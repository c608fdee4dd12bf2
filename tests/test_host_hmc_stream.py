"""The premises of tests/test_gpu_hmc_stream.py, asserted on the oracle alone (no GPU): for every case of
hmc_stream.CASES the probe is exact on the oracle, the oracle's Gaussians stay inside the bound that the device is held to,
and the inputs have the properties that make the comparison sharp (NOTES/hmc-stream.md)."""
import ctypes as C

import numpy as np
import pytest

import hmc_stream as H

CASE_NAMES = [c["name"] for c in H.CASES]


def test_long_double_is_wider_than_double():
    """the reference is only a reference where numpy.longdouble carries more than 53 bits"""
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("seed,word,second", [H.ZERO_WORD_SECOND + (True,), H.ZERO_WORD_FIRST + (False,)])
def test_zero_word_seeds(oracle, seed, word, second):
    """the two seeds found by scripts/find_zero_word_seeds.py, re-derived with ora_rng_get: the named output word of a fresh
    stream is 0 and no earlier one is; in a first block of 210 values it is skipped, as the first or as the second word of the
    pair it would have belonged to"""
    L = oracle.lib()
    r = oracle.Rng()
    L.ora_rng_set(C.byref(r), seed)
    w = [L.ora_rng_get(C.byref(r)) for _ in range(624)]
    assert w[word] == 0 and all(v != 0 for v in w[:word])
    b = H.draw_block(H.Words(oracle, seed), 0, 210)
    assert b["zero"] and b["zero_at"] == [word]
    assert b["begin"] == 0 and b["begin"] + 4 * 210 > word
    # no zero before it: the pairs before it are (0, 1), (2, 3), ...; the pair that meets it begins at word - 1 or at word
    assert (word % 2 == 1) == second
    firsts = b["pair_first"]
    assert ((word - 1) in firsts) if second else ((word + 1) in firsts and word not in firsts)
    # the product's host stream (orc_host_gsl_stream: the specification of the perturbation, tests/test_gpu_multistart.py) skips
    # it as the oracle's does, and both give the replay's values
    from or_cdchomp_amd import _capi
    host = np.zeros(210); hu = np.zeros(1)
    assert _capi.lib().orc_host_gsl_stream(seed, 0.1, 210, host.ctypes.data_as(_capi.c_double_p), hu.ctypes.data_as(_capi.c_double_p)) == 0
    L.ora_rng_set(C.byref(r), seed)
    ora = np.array([L.ora_ran_gaussian(C.byref(r), 0.1) for _ in range(210)])
    assert np.array_equal(host, ora) and hu[0] == L.ora_rng_uniform(C.byref(r))
    assert H.ulp_error(ora, b["ref"] * H.LD(0.1) / H.sigma_ld(0)).max() <= H.ULP_BOUND


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_probe_is_exact_on_the_oracle(oracle, name):
    """lambda_ 1e300 (1e30): the oracle's AG after each call equals the replay's last block bit for bit, its trajectory equals
    the seed, its status is 0 and its schedule the replay's; the oracle's values lie within the bound of the long-double
    reference"""
    c = H.CASE[name]
    rep = H.replay_case(oracle, c)
    ora = H.oracle_case(oracle, c)
    ref = H.reference_ag(oracle, c)
    L = oracle.lib()
    worst = 0.0
    for k, seed in enumerate(H.case_seeds(c)):
        # the blocks by the oracle's own generator, from a stream of their own
        r = oracle.Rng()
        L.ora_rng_set(C.byref(r), int(seed))
        last = None
        for q, call in enumerate(rep[k]):
            for b in call["blocks"]:
                last = np.array([L.ora_ran_gaussian(C.byref(r), b["sigma"]) for _ in range(H.case_mn(c))])
                assert L.ora_rng_uniform(C.byref(r)) == b["u"]
            assert last is not None, "a run draws its first block at iteration 0 of its first call"
            assert np.array_equal(ora["ag"][q, k], last), (name, k, q)
            assert ora["next"][q, k] == call["next"], (name, k, q)
            if not c["floating"]:
                assert ora["traj_same"][q, k], (name, k, q)
            assert ora["status"][q, k] == 0
            err = H.ulp_error(ora["ag"][q, k], ref[q][k]).max()
            worst = max(worst, err)
            assert err <= H.ULP_BOUND, (name, k, q, err)
    print("%s: the oracle's worst distance from the long-double reference %.2f ulp" % (name, worst))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_conditions_on_the_inputs(oracle, name):
    """no schedule quotient within 1e-9 of an integer (a one-ulp log cannot move a resample), no u of 0; for an fp32 case
    no reference value within 8 double ulp of a float rounding tie"""
    c = H.CASE[name]
    rep = H.replay_case(oracle, c)
    blocks = [b for run in rep for call in run for b in call["blocks"]]
    assert blocks
    for b in blocks:
        assert b["u"] > 0.0
        assert abs(b["quotient"] - round(b["quotient"])) >= 1e-9, b["quotient"]
    if c["precision"] == 32:
        for ref in H.reference_ag(oracle, c):
            assert H.tie_distance(ref).min() > H.ULP_BOUND
            assert np.all(np.abs(ref.astype(np.float64)) > 1e-30)      # far from float's subnormals


def test_what_the_cases_cover(oracle):
    """over the table: at least 10 blocks with a pair that began on word 623 of a state (the carry across a twist); the two
    zero-word seeds skip their word inside the first block of the first case; every block length begins blocks at both word
    parities; the calls resample where the case says"""
    rep = {c["name"]: H.replay_case(oracle, c) for c in H.CASES}
    carries = sum(b["carry"] for runs in rep.values() for run in runs for call in run for b in call["blocks"])
    print("blocks with a pair begun on word 623:", carries)
    assert carries >= 10
    first = rep["first_block"]
    seeds = H.case_seeds(H.CASE["first_block"])
    for seed, word in (H.ZERO_WORD_SECOND, H.ZERO_WORD_FIRST):
        b = first[seeds.index(seed)][0]["blocks"][0]
        assert b["zero_at"] == [word]
    assert not any(first[k][0]["blocks"][0]["zero"] for k, s in enumerate(seeds) if s not in (H.ZERO_WORD_SECOND[0], H.ZERO_WORD_FIRST[0]))
    assert np.array_equal(first[0][0]["blocks"][0]["ref"], first[1][0]["blocks"][0]["ref"])            # seed 0 is 4357
    for name in ("every_iteration", "every_iteration_fp32"):
        for run in rep[name]:
            assert [b["iteration"] for b in run[0]["blocks"]] == list(range(12))
            assert [b["iteration"] for b in run[1]["blocks"]] == list(range(12, 20))
    for name in ("length_7", "length_238", "length_245", "length_252", "length_686"):
        parities = {b["begin"] % 2 for run in rep[name] for b in run[0]["blocks"]}
        assert parities == {0, 1}, name
        for run in rep[name]:
            assert len(run[0]["blocks"]) == 6
    for name in ("sparse_0.3", "sparse_0.05"):
        counts = np.array([[len(call["blocks"]) for call in run] for run in rep[name]])
        print(name, "resamples per run and call:", counts.tolist())
        assert (counts[:, 0] == 1).all()
        assert counts[:, 1:].sum() >= 8
        if name == "sparse_0.05":
            assert (counts[:, 1:] == 0).any()          # a call that draws nothing leaves an older block in AG
    # a block of 686 values spans three twists
    b = rep["length_686"][0][0]["blocks"][1]
    end = rep["length_686"][0][0]["blocks"][2]["begin"]
    assert end // 624 - b["begin"] // 624 >= 2
