"""Host: the library's counter-based generator (csrc/sg_rng.hpp) and the layout its consumers document, without a GPU.

tests/rng_ref.py restates the generator in numpy uint64.  Here it is held to the published splitmix64 sequence, to the header's
own __host__ functions (through the test library's sg_test_rng_host, which makes no device call), and to simgan_amd.utils.
derive_seed; the consumers' (seed, stream, counter) layout is checked for stream hygiene; and the comparison the GPU suite makes
(tests/test_gpu_rng.py) is shown to catch four layout defects that the moment / frequency assertions it stands beside let through.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rng_ref as rr  # noqa: E402

M64 = rr.M64


# ------------------------------------------------------------------------------------------------ the generator itself
def test_mix64_is_splitmix64():
    """The published splitmix64 outputs from state 0: output i is the finaliser of state i * gamma, and sg_mix64 adds one gamma
    itself, so sg_mix64(i * gamma) is output i + 1 of the sequence."""
    gamma = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [rr.mix64_int((i * gamma) & M64) for i in range(3)] == want
    assert [int(v) for v in rr.mix64([(i * gamma) & M64 for i in range(3)])] == want


def test_numpy_and_integer_restatements_agree():
    rng = np.random.default_rng(0)
    xs = [0, 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1] + [int(v) for v in rng.integers(0, 1 << 64, 200, dtype=np.uint64)]
    assert [int(v) for v in rr.mix64(xs)] == [rr.mix64_int(x) for x in xs]
    for seed, stream, ctr in zip(xs, xs[::-1], xs[3:] + xs[:3]):
        want = rr.mix64_int((rr.mix64_int(seed ^ ((stream * rr.STREAM_MUL) & M64)) + ctr) & M64)
        assert int(rr.key(seed, stream, ctr)[0]) == want


def _host_lib():
    from simgan_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        raise AssertionError("libsimgan_hip_test.so missing: run __graft_entry__.build()")
    lib = C.CDLL(_lib.TEST_LIB_PATH)
    res, args = _lib.TEST_PROTOTYPES["sg_test_rng_host"]
    lib.sg_test_rng_host.restype, lib.sg_test_rng_host.argtypes = res, args
    return lib


def host_draw(lib, kind, n, seed, stream, ctr0=0):
    out = np.empty(n, np.int64 if kind == 0 else np.float32)
    assert lib.sg_test_rng_host(kind, n, seed & M64, stream & M64, ctr0 & M64, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def triples():
    """(seed, stream, ctr0): the product's streams, values >= 2^63, and seeds / counters that wrap at 2^64."""
    rng = np.random.default_rng(1)
    big = [int(v) | (1 << 63) for v in rng.integers(0, 1 << 64, 6, dtype=np.uint64)]
    t = [(0, 0, 0), (M64, rr.SG_ACT_STREAM, 0), (M64, M64, M64 - 5), (big[0], big[1], big[2]), (big[3], 3 * rr.PPO_EPOCH_MUL + 1, big[4]),
         (rr.call_seed(M64, 2), rr.DISC_PPERM_STREAM + 1024, 0), (big[5], rr.SG_KFAC_STREAM + 1, (1 << 32) - 3)]
    t += [tuple(int(v) for v in rng.integers(0, 1 << 64, 3, dtype=np.uint64)) for _ in range(8)]
    return t


def test_call_seed_wraps_like_the_python_side():
    assert rr.call_seed(M64, 1) == 0 and rr.call_seed(M64, 2) == 1 and rr.call_seed(5, 3) == 8
    assert rr.call_seed(M64 - 1, 1) == M64


def test_uniform_equals_the_headers_host_function():
    lib = _host_lib()
    for seed, stream, ctr0 in triples():
        n = 4099
        got = host_draw(lib, 1, n, seed, stream, ctr0)
        want = rr.uniform(seed, stream, (np.arange(n, dtype=np.uint64) + np.uint64(ctr0)))
        assert np.array_equal(got, want), (seed, stream, ctr0)
        assert got.min() >= 0.0 and got.max() < 1.0


@pytest.mark.parametrize("n", [1, 2, 35, 77, 4096, 4097])
def test_permutation_equals_the_headers_host_function(n):
    """4096 is the whole Feistel domain at half_bits 6: no cycle walking.  4097 is the smallest n of the next domain (16384):
    about 3/4 of the first applications fall outside [0, n) and walk on."""
    lib = _host_lib()
    assert rr.perm_half_bits(n) == {1: 1, 2: 1, 35: 3, 77: 4, 4096: 6, 4097: 7}[n]
    for seed, stream, _ in triples():
        got = host_draw(lib, 0, n, seed, stream)
        want = rr.fill_perm(n, seed, stream)
        assert np.array_equal(got, want), (n, seed, stream)
        assert np.array_equal(np.sort(want), np.arange(n))
        hits = rr.first_hits(n, rr.perm_key(seed, stream))
        if n == 4096:
            assert hits == n
        if n == 4097:
            assert 0.15 * n < hits < 0.35 * n, hits   # 4097 / 16384 = 0.25 of a bijection's images, +- 10 binomial sigma


def test_normal64_is_box_muller_on_the_keys_bits():
    """u1 in (0, 1] from the top 24 bits (+ 1), u2 in [0, 1) from bits 16..39: the bit fields do not overlap, both are exact in
    float32, and the float64 formula has the moments of a standard normal."""
    ctr = np.arange(1 << 16, dtype=np.uint64)
    k = rr.key(5, 9, ctr)
    u1, u2 = rr.normal_uniforms(5, 9, ctr)
    assert np.array_equal(u1, (((k >> np.uint64(40)).astype(np.float64)) + 1) / 2.0 ** 24)
    assert np.array_equal(u2, ((k >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    z = rr.normal64(5, 9, ctr)
    assert np.isfinite(z).all() and abs(z.mean()) < 5 / 256 and abs(z.std() - 1) < 5 / 362   # 5 sigma of 2^16 draws
    assert np.abs(rr.normal32(5, 9, ctr) - z).max() < 1e-5


def test_scan_finds_both_ends_of_u1():
    """The counters tests/test_gpu_rng.py evaluates sg_normal at: u1 = 2^-24 gives the generator's largest |z|, u1 = 1 gives 0."""
    seed, stream = 0x5EED5EED, rr.SG_ACT_STREAM
    lo, hi = rr.find_u1_ends(seed, stream)
    assert (lo, hi) == (52613753, 15430582)
    u1, u2 = rr.normal_uniforms(seed, stream, [lo, hi])
    assert u1[0] == 2.0 ** -24 and u1[1] == 1.0
    z = rr.normal64(seed, stream, [lo, hi])
    assert z[1] == 0.0 and abs(abs(z[0]) - np.sqrt(48 * np.log(2.0)) * abs(np.cos(rr.TWO_PI_F32 * u2[0]))) < 1e-12
    assert np.abs(rr.normal32(seed, stream, [lo, hi]) - z).max() < 1e-5


def test_derive_seed_restated():
    from simgan_amd import utils
    for seed, salt in ((0, rr.SALT_PPO), (7, rr.SALT_DISC), (M64, rr.SALT_ACKTR), (123456789, 1)):
        assert utils.derive_seed(seed, salt) == rr.derive_seed(seed, salt)
    before = utils._INSTANCES[0]
    got = utils.derive_seed(3, rr.SALT_POLICY, per_instance=True)
    assert utils._INSTANCES[0] == before + 1 and got == rr.derive_seed(3, rr.SALT_POLICY, before + 1)
    assert got < 1 << 62


# ------------------------------------------------------------------------------------------------ stream hygiene
CALLS, RANKS, EPOCHS = 1000, 8, 10


def _default_objects():
    """Seeds of default-constructed objects (constructor seed 0) in one process: Policy, SplitPolicy, a second Policy and a
    PolicyEnsemble take instance numbers as they are built -- a policy's constructor derives twice (the handle's provisional
    seed, then the constructor's), so the four objects hold instance numbers 2, 4, 6 and 7; any other building order gives other
    small numbers, so every instance number 1..16 is covered for both per-instance salts."""
    seeds = {f"policy#{i}": rr.derive_seed(0, rr.SALT_POLICY, i) for i in range(1, 17)}
    seeds.update({f"ensemble#{i}": rr.derive_seed(0, rr.SALT_ENSEMBLE, i) for i in range(1, 17)})
    seeds.update({"ppo": rr.derive_seed(0, rr.SALT_PPO), "acktr": rr.derive_seed(0, rr.SALT_ACKTR), "disc": rr.derive_seed(0, rr.SALT_DISC)})
    return seeds


def _all_stream_keys():
    """{label: uint64 array} of every first-level key sg_mix64(seed ^ stream * STREAM_MUL) the consumers reach over the first
    CALLS calls, RANKS ranks and EPOCHS epochs, and for the permutations (whose stream is PERM_STREAM and whose caller's stream
    id is the COUNTER) also the second-level argument stream_key + stream_id, which is what tells two permutations apart."""
    seeds = _default_objects()
    calls = np.arange(1, CALLS + 1, dtype=object)
    out = {}
    for name, s in seeds.items():
        if name.startswith(("policy", "ensemble")):
            for r in range(RANKS):
                out[f"{name} act rank {r}"] = rr.stream_key([rr.call_seed(s, c) for c in calls], rr.SG_ACT_STREAM + r)
    s = seeds["ppo"]
    first = rr.stream_key([rr.call_seed(s, c) for c in calls], rr.PERM_STREAM)
    out["ppo perm stream"] = first
    for e in range(EPOCHS):
        for r in range(RANKS):
            out[f"ppo perm epoch {e} rank {r}"] = first + np.uint64(rr.ppo_perm_layout(s, 1, e, r)[1])
    s = seeds["disc"]
    cs = [rr.call_seed(s, c) for c in calls]
    dfirst = rr.stream_key(cs, rr.PERM_STREAM)
    out["disc perm stream"] = dfirst
    k = np.arange(1, CALLS + 1, dtype=np.uint64)          # rng_calls == calls when every call is an update epoch
    out["disc eperm"] = dfirst + (np.uint64(rr.DISC_EPERM_STREAM) + k)
    for r in range(RANKS):
        out[f"disc pperm rank {r}"] = dfirst + (np.uint64(rr.DISC_PPERM_STREAM) + k * np.uint64(1024) + np.uint64(r))
    out["disc alpha"] = rr.stream_key(cs, np.uint64(rr.DISC_ALPHA_STREAM) + k)
    out["disc grad pen"] = rr.stream_key(cs, rr.GRAD_PEN_STREAM)
    out["acktr noise"] = rr.stream_key(seeds["acktr"], np.uint64(rr.SG_KFAC_STREAM) + np.arange(CALLS, dtype=np.uint64))
    return out


def test_first_level_keys_are_pairwise_distinct():
    keys = _all_stream_keys()
    perms = np.concatenate([v for k, v in keys.items() if " perm epoch" in k or "eperm" in k or "pperm" in k])
    streams = np.concatenate([v for k, v in keys.items() if " perm" not in k and "eperm" not in k and "pperm" not in k])
    firsts = np.concatenate([streams, keys["ppo perm stream"], keys["disc perm stream"]])
    assert streams.size > 250000 and perms.size == CALLS * (EPOCHS * RANKS + 1 + RANKS)
    assert np.unique(firsts).size == firsts.size      # first-level keys: consumers x calls x ranks
    assert np.unique(perms).size == perms.size        # what a permutation is keyed by: consumers x calls x epochs x ranks
    # A draw is sg_mix64(first-level key + counter), a permutation's key sg_mix64(first-level key + stream id): two streams
    # whose keys lie closer than the counters reach, or a permutation's argument inside a stream's counters, would share values.
    # None does within 2^22 counters (16 steps x 16384 environments x 16 action dimensions in one call).
    span = np.uint64(1 << 22)
    s = np.sort(streams)
    assert int(np.diff(s).min()) > int(span), int(np.diff(s).min())
    below = s[np.searchsorted(s, perms, side="right") - 1]     # the stream key at or below each permutation argument (wraps to the last)
    assert not np.any(perms - below <= span)


def test_learner_and_inner_halves_of_the_chained_act_differ():
    """The chain's learner half draws on policy.seed + policy._act_calls, the inner half on ensemble.seed + ensemble._calls, both
    on SG_ACT_STREAM + rank: the salts (and the instance numbers) keep them apart at every pair of call numbers."""
    for i in range(1, 9):
        for j in range(1, 9):
            ps, es = rr.derive_seed(0, rr.SALT_POLICY, i), rr.derive_seed(0, rr.SALT_ENSEMBLE, j)
            assert abs(ps - es) > 2 * CALLS   # no (call, call') makes the two seeds meet
            a = rr.normal64(*rr.act_layout(ps, 1, 0, 16, 12))
            b = rr.normal64(*rr.act_layout(es, 1, 0, 16, 12))
            assert not np.any(a == b)


def test_disc_policy_permutation_stream_does_not_alias_below_1024_ranks():
    """stream_id = 0xF0000000 + rng_calls * 1024 + rank is injective in (rng_calls, rank) for rank < 1024, stays clear of the
    expert permutation's 0xE0000000 + rng_calls over the first 2^28 / 1024 epochs, and alpha's 0xA1000000 + rng_calls stays
    clear of the grad-pen stream 0xA2000000 for 2^24 epochs."""
    k = np.arange(1, CALLS + 1, dtype=np.uint64)[:, None]
    r = np.arange(1024, dtype=np.uint64)[None, :]
    ids = (np.uint64(rr.DISC_PPERM_STREAM) + k * np.uint64(1024) + r).reshape(-1)
    assert np.unique(ids).size == ids.size
    assert int(ids.min()) > rr.DISC_EPERM_STREAM + CALLS and rr.DISC_ALPHA_STREAM + CALLS < rr.GRAD_PEN_STREAM
    assert [rr.disc_layout(0, 1, 2, rank=1023, sharded=True)["pperm"][1] + 1] == [rr.disc_layout(0, 1, 3, rank=0, sharded=True)["pperm"][1]]
    assert rr.disc_layout(0, 1, 2, rank=5, sharded=False)["pperm"][1] == rr.disc_layout(0, 1, 2, rank=0, sharded=True)["pperm"][1]
    # ... and rank 1024 WOULD alias the next epoch's rank 0: the bound of the layout, stated
    assert rr.DISC_PPERM_STREAM + 2 * 1024 + 1024 == rr.DISC_PPERM_STREAM + 3 * 1024 + 0


# ------------------------------------------------------------------------------------------------ tests of the test
N_ROWS, A_DIM, SEED = 256, 12, rr.derive_seed(0, rr.SALT_POLICY, 2)


def gaussian_noise(call, rank, defect=None, n=N_ROWS, A=A_DIM):
    """The [n, A] standard normals of one act call as the layout has them, or with one layout defect."""
    seed, stream, ctr = rr.act_layout(SEED, call, rank, n, A)
    row, col = np.divmod(ctr, np.uint64(A))
    if defect == "tile":            # every 16-row tile draws what tile 0 drew
        ctr = (row % np.uint64(16)) * np.uint64(A) + col
    elif defect == "columns":       # one draw per row, shared by its A columns
        ctr = row * np.uint64(A)
    elif defect == "pass":          # the counter restarts at the second 128-row pass
        ctr = (row % np.uint64(128)) * np.uint64(A) + col
    elif defect == "rank":          # the rank does not reach the stream
        stream = rr.SG_ACT_STREAM
    return rr.normal64(seed, stream, ctr).astype(np.float32)


def old_gaussian_predicates(z1, z2):
    """tests/test_gpu_parity.py::test_policy_library_rng's assertions on the draws, verbatim (z = (a1 - mean) / std; with a
    state-independent std, a1 != a2 is z1 != z2)."""
    z = z1
    return (not np.allclose(z1, z2)) and abs(z.mean()) < 0.3 and 0.7 < z.std() < 1.3


def new_gaussian_comparison(z, call, rank):
    """What tests/test_gpu_rng.py asserts: the consumer's draws ARE the generator's at the documented layout."""
    return np.array_equal(z, rr.normal64(*rr.act_layout(SEED, call, rank, *z.shape)).astype(np.float32))


@pytest.mark.parametrize("defect", ["tile", "columns", "pass", "rank"])
def test_layout_defects_pass_the_moment_assertions_and_fail_the_comparison(defect):
    rank = 1   # (rank 0 cannot show a missing rank term)
    assert old_gaussian_predicates(gaussian_noise(1, rank), gaussian_noise(2, rank))
    assert new_gaussian_comparison(gaussian_noise(1, rank), 1, rank) and new_gaussian_comparison(gaussian_noise(2, rank), 2, rank)
    z1, z2 = gaussian_noise(1, rank, defect), gaussian_noise(2, rank, defect)
    assert old_gaussian_predicates(z1, z2), "the defect is one the moment assertions let through"
    assert not new_gaussian_comparison(z1, 1, rank) and not new_gaussian_comparison(z2, 2, rank)
    if defect == "rank":   # "the same noise on every rank": passes rank by rank, and only the comparison sees it
        assert np.array_equal(z1, gaussian_noise(1, 0))


def bernoulli_bits(call, rank, p, n, defect=None):
    seed, stream, ctr = rr.act_layout(SEED, call, rank, n, p.size)
    K = np.uint64(p.size)
    if defect == "columns":
        ctr = (ctr // K) * K
    elif defect in ("tile", "pass"):
        ctr = ((ctr // K) % np.uint64(16 if defect == "tile" else 128)) * K + ctr % K
    elif defect == "rank":
        stream = rr.SG_ACT_STREAM
    return (rr.uniform(seed, stream, ctr.reshape(-1)).reshape(n, p.size) < p[None, :]).astype(np.float32)


def old_frequency_predicates(a, a2, p, n):
    """tests/test_gpu_discrete.py::test_library_draws_follow_the_probabilities' assertions (Bernoulli), verbatim."""
    freq = a.mean(0)
    bad = np.abs(freq - p) > 5 * np.sqrt(p * (1 - p) / n)
    return set(np.unique(a).tolist()) <= {0.0, 1.0} and not bad.any() and not np.array_equal(a, a2)


@pytest.mark.parametrize("defect", ["columns", "rank"])
def test_layout_defects_pass_the_frequency_assertions_and_fail_the_comparison(defect):
    """65,536 copies of one observation, as that test has them.  (Draws repeated per 16-row tile or per 128-row pass leave 16 or
    128 distinct rows, which its 5 sigma bound at n = 65,536 does reject: those two are the moment assertions' blind spot,
    above.)"""
    n, rank = 65536, 1
    p = np.array([0.11, 0.5, 0.73, 0.9, 0.32])
    good = bernoulli_bits(1, rank, p, n)
    assert old_frequency_predicates(good, bernoulli_bits(2, rank, p, n), p, n)
    a, a2 = bernoulli_bits(1, rank, p, n, defect), bernoulli_bits(2, rank, p, n, defect)
    assert old_frequency_predicates(a, a2, p, n), "the defect is one the frequency assertions let through"
    assert not np.array_equal(a, good)
    for other in ("tile", "pass"):
        assert not old_frequency_predicates(bernoulli_bits(1, rank, p, n, other), bernoulli_bits(2, rank, p, n, other), p, n)
