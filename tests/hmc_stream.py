"""The device-drawn GSL streams of hmc runs held to the stream itself (NOTES/hmc-stream.md): what tests/test_host_hmc_stream.py
and tests/test_gpu_hmc_stream.py share.

The probe.  In a momentum iteration AG is the resampled noise plus (0.5 / lambda) A^-1 G, and then T -= AG / lambda.  With
lambda_ = 1e300 (1e30 for an fp32 batch) both terms vanish below one ulp, so AG after an iterate call IS the last noise block
that the call, or an earlier one, drew, and the trajectory stays the seed.  A block at the end of a call depends on every word
of the stream consumed before it and on every resample iteration before its own.

The replay of a run is made from the stream's WORDS (ora_rng_get) and follows run_iterate: `iter` restarts at 0 in every call,
the next resample iteration persists.  The reference value of an entry is evaluated in long double from the same words: x, y
and r2 in double, as the specification forms them, everything after that -- the logarithm, the quotient, the square root, the
two products and sigma = 1 / sqrt(100 exp(0.02 iter)) -- in numpy.longdouble.

The bound, 8 ulp of the value in fp64, is derived and not measured: exp, the product, sqrt and the reciprocal give sigma within
about 1.75 ulp; log, the quotient and sqrt give about 1.25 ulp; the two products bring the total to about 4 ulp; doubling that
allows for a 1 ulp log and exp on the device.  An fp32 batch is asked for float32(reference) exactly, on the condition that no
reference value lies within 8 double ulp of a float rounding tie (asserted on the host)."""
import ctypes as C
import functools

import numpy as np

import common

LD = np.longdouble
ULP_BOUND = 8.0

# Seeds whose fresh stream holds a zero output word (scripts/find_zero_word_seeds.py), which gsl_rng_uniform_pos skips and the
# wavefront's 64-pair chunk hands to its one-at-a-time walk.  Counted from 0:
ZERO_WORD_SECOND = (7603642, 141)       # the second word of its pair
ZERO_WORD_FIRST = (7627928, 400)        # the first word of its pair

FIRST_BLOCK_SEEDS = [0, 4357, 1, 2, 0xFFFFFFFF, ZERO_WORD_SECOND[0], ZERO_WORD_FIRST[0], 12345, 3]


def case(name, n_runs, n_points, lam, calls, precision=64, floating=False, seeds="arange", seed0=0):
    if seeds == "arange":
        seeds = [seed0 + k for k in range(n_runs)]
    return dict(name=name, n_runs=n_runs, n_points=n_points, lam=lam, calls=tuple(calls), precision=precision, floating=floating,
                seeds=None if seeds is None else tuple(int(s) for s in seeds))


# The smallest shapes at which each mechanism exists.  n = 7 (the WAM with a fixed base) but for the last: values per block
# 7 (n_points - 2).
CASES = [
    # 9 runs: the last workgroup of four wavefronts has one.  210 values.  Runs 0 and 1 are the same stream (GSL seeds 0 as 4357)
    case("first_block", 9, 32, 0.3, [1], seeds=FIRST_BLOCK_SEEDS),
    case("first_block_no_seeds", 9, 32, 0.3, [1], seeds=None),
    # a resample in every iteration; the second call resamples from iteration 12 on only (the persisted schedule)
    case("every_iteration", 8, 12, 50.0, [12, 20], seed0=10),
    case("every_iteration_fp32", 8, 12, 50.0, [12, 20], precision=32, seed0=10),
    case("sparse_0.3", 8, 12, 0.3, [1, 15, 40], seed0=20),
    case("sparse_0.05", 8, 12, 0.05, [1, 15, 40], seed0=30),
    # 7: the smallest create accepts; 238, 245, 252 straddle the ~245 Gaussians of one state; 686 spans three twists
    case("length_7", 4, 3, 50.0, [6], seed0=40),
    case("length_238", 4, 36, 50.0, [6], seed0=50),
    case("length_245", 4, 37, 50.0, [6], seed0=60),
    case("length_252", 4, 38, 50.0, [6], seed0=70),
    case("length_686", 4, 100, 50.0, [6], seed0=80),
    # 256 runs and more: the device streams without a switch
    case("default_trigger", 260, 12, 50.0, [6], seed0=1000),
    # the config-4 shape: base pose in columns 0..6
    case("floating_base", 4, 12, 50.0, [6], floating=True, seed0=90),
]
CASE = {c["name"]: c for c in CASES}


def case_n(c):
    return 14 if c["floating"] else 7


def case_mn(c):
    return (c["n_points"] - 2) * case_n(c)


def case_lambda(c):
    return 1e300 if c["precision"] == 64 else 1e30


def case_kw(c):
    kw = dict(n_points=c["n_points"], lambda_=case_lambda(c), obs_factor=500.0, use_momentum=1, use_hmc=1, hmc_resample_lambda=c["lam"])
    if c["floating"]:
        kw["floating_base"] = 1
    return kw


def case_seeds(c):
    """the seed of every run as the stream sees it (no seeds given: 0)"""
    return [0] * c["n_runs"] if c["seeds"] is None else list(c["seeds"])


def case_goals(c):
    """(goals [n_runs][7], basegoals [n_runs][7] or None)"""
    goals = common.wam_goals(c["n_runs"], seed=20250103)
    if not c["floating"]:
        return goals, None
    _, base, _, _ = common.wam_state()
    basegoals = np.tile(np.asarray(base, dtype=np.float64), (c["n_runs"], 1))
    basegoals[:, :3] += np.random.default_rng(20250103).uniform(-0.3, 0.3, size=(c["n_runs"], 3))
    return goals, basegoals


# ---- the stream, word by word ----------------------------------------------------------------------------------------
class Words:
    """the output words of one GSL stream (ora_rng_get), kept so that a position can be read again"""

    def __init__(self, oracle, seed):
        self._get = oracle.lib().ora_rng_get
        self._r = oracle.Rng()
        oracle.lib().ora_rng_set(C.byref(self._r), int(seed))
        self._ref = C.byref(self._r)
        self.w = np.zeros(0, dtype=np.int64)
        self.pos = 0

    def window(self, count):
        """the words [pos, pos + count)"""
        end = self.pos + count
        if end > self.w.size:
            more = max(end - self.w.size, 4096)
            get, ref = self._get, self._ref
            self.w = np.concatenate([self.w, np.array([get(ref) for _ in range(more)], dtype=np.int64)])
        return self.w[self.pos:end]


def sigma_ld(it):
    """1 / sqrt(100 exp(0.02 it)) in long double from the double constants (src/orcdchomp_mod.cpp:2759-2762)"""
    return LD(1) / np.sqrt(LD(100.0) * np.exp(LD(0.02) * LD(it)))


def draw_block(words, it, mn):
    """mn values of gsl_ran_gaussian(sigma(it)) from `words`, which moves behind the pair of the last one.  Returns a dict:
    ref [mn] long double; sigma (the double the specification passes); begin (the word position of the block); carry (an
    attempted pair began on word 623 of a state); zero (a zero word was skipped inside it)"""
    begin = words.pos
    count = 4 * mn + 256
    while True:
        w = words.window(count)
        nz = np.flatnonzero(w != 0)
        pairs = nz.size // 2
        i1, i2 = nz[0:2 * pairs:2], nz[1:2 * pairs:2]
        x = -1 + 2 * (w[i1] / 4294967296.0)
        y = -1 + 2 * (w[i2] / 4294967296.0)
        r2 = x * x + y * y
        acc = ~((r2 > 1.0) | (r2 == 0))
        if acc.sum() >= mn:
            break
        count *= 2
    last = int(np.flatnonzero(acc)[mn - 1])              # the pair of the last value wanted
    used = int(i2[last]) + 1
    keep = np.flatnonzero(acc)[:mn]
    yl, rl = y[keep].astype(LD), r2[keep].astype(LD)
    ref = sigma_ld(it) * yl * np.sqrt(LD(-2.0) * np.log(rl) / rl)
    out = dict(iteration=it, begin=begin, ref=ref, sigma=1.0 / np.sqrt(100.0 * np.exp(0.02 * it)),
               carry=bool((((begin + i1[:last + 1]) % 624) == 623).any()), zero=bool((w[:used] == 0).any()),
               zero_at=[begin + int(z) for z in np.flatnonzero(w[:used] == 0)], pair_first=[begin + int(z) for z in i1[:last + 1]])
    words.pos += used
    return out


def replay_run(oracle, seed, calls, mn, lam):
    """one run over a list of iterate calls: per call the list of its blocks (draw_block's dicts, with `u` and `quotient` =
    -log(u) / lam of the uniform behind the block), and the schedule left behind"""
    words = Words(oracle, seed)
    nxt = 0
    out = []
    for n_iter in calls:
        blocks = []
        for it in range(n_iter):
            if it != nxt:
                continue
            b = draw_block(words, it, mn)
            u = float(words.window(1)[0]) / 4294967296.0
            words.pos += 1
            b["u"] = u
            b["quotient"] = (-np.log(u) / lam) if u > 0 else np.inf
            if u > 0:
                nxt += 1 + int(b["quotient"])
            blocks.append(b)
        out.append(dict(blocks=blocks, next=nxt))
    return out


@functools.lru_cache(maxsize=None)
def _replay_case(oracle, name):
    c = CASE[name]
    memo = {}
    runs = []
    for seed in case_seeds(c):
        key = 4357 if seed == 0 else seed
        if key not in memo:
            memo[key] = replay_run(oracle, seed, c["calls"], case_mn(c), c["lam"])
        runs.append(memo[key])
    return runs


def replay_case(oracle, c):
    """[n_runs][n_calls] of replay_run's dicts, computed once"""
    return _replay_case(oracle, c["name"])


def last_block(replayed_run, call):
    """the block AG holds after `call`: the last one that the call, or an earlier one, drew"""
    for q in range(call, -1, -1):
        if replayed_run[q]["blocks"]:
            return replayed_run[q]["blocks"][-1]
    return None


def reference_ag(oracle, c):
    """[n_calls][n_runs][mn] long double: AG after every call by the replay"""
    rep = replay_case(oracle, c)
    return [np.stack([last_block(rep[k], q)["ref"] for k in range(c["n_runs"])]) for q in range(len(c["calls"]))]


# ---- the oracle's runs -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(oracle, name):
    c = CASE[name]
    model, base, dofvals, adofs = common.wam_state()
    prob = _problem(oracle)
    goals, basegoals = case_goals(c)
    rob = oracle.OraRobot(model)
    m, n = c["n_points"] - 2, case_n(c)
    ag = np.zeros((len(c["calls"]), c["n_runs"], m * n))
    nxt = np.zeros((len(c["calls"]), c["n_runs"]), dtype=np.int64)
    status = np.zeros((len(c["calls"]), c["n_runs"]), dtype=np.int64)
    traj_same = np.ones((len(c["calls"]), c["n_runs"]), dtype=bool)
    for k, seed in enumerate(case_seeds(c)):
        p = oracle.default_params(seed=int(seed), **case_kw(c))
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], p,
                            basegoal=None if basegoals is None else basegoals[k])
        assert run.n == n and run.m == m
        seed_traj = run.traj().copy()
        for q, n_iter in enumerate(c["calls"]):
            status[q, k], _ = run.iterate(n_iter)
            ag[q, k] = run.mat("AG", m, n).reshape(-1)
            nxt[q, k] = oracle.lib().ora_run_hmc_resample_iter(run.h)
            traj_same[q, k] = np.array_equal(run.traj(), seed_traj)
        run.destroy()
    return dict(ag=ag, next=nxt, status=status, traj_same=traj_same)


@functools.lru_cache(maxsize=None)
def _problem(oracle):
    return common.tabletop_problem(oracle)


def oracle_case(oracle, c):
    """the oracle's runs of the case, once: ag [n_calls][n_runs][mn], next (hmc_resample_iter), status, traj_same (the
    trajectory equals the seed) [n_calls][n_runs]"""
    return _oracle_case(oracle, c["name"])


# ---- distances ---------------------------------------------------------------------------------------------------------
def ulp_error(got, ref):
    """|got - ref| in units of the double spacing at ref, ref long double"""
    ref = np.asarray(ref, dtype=LD)
    sp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / sp).astype(np.float64)


def tie_distance(ref):
    """the distance of every long-double reference value from the nearer float rounding tie, in double ulp of the value"""
    ref = np.asarray(ref, dtype=LD)
    f = ref.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64).astype(LD)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64).astype(LD)
    fl = f.astype(np.float64).astype(LD)
    d = np.minimum(np.abs(ref - (fl + up) / 2), np.abs(ref - (fl + dn) / 2))
    return (d / np.spacing(np.abs(ref.astype(np.float64))).astype(LD)).astype(np.float64)
