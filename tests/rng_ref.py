"""Host restatement of csrc/sg_rng.hpp and of the layout every consumer of it documents.

The generator is counter-based and stateless: value = f(seed, stream, counter).  Its integer part -- sg_mix64, sg_key, the 24
bits of sg_uniform, sg_feistel / sg_perm_at with cycle walking -- is uint64 arithmetic modulo 2^64, which numpy reproduces bit
for bit; only sg_normal goes through logf / cosf / sqrtf, and `normal64` states it in float64 from the same key.

The second half states WHICH (seed, stream, counters) feed which element of which consumer, as the consumers' own comments have
it (sg_policy.hip, sg_policy_fwd.hpp, sg_act_step.hip:19, sg_act_chain.hip, sg_ppo.hip: sg_fill_perm and its three callers,
sg_disc.hip, sg_kfac.hpp, and the Python side's `(obj.seed + calls) & (2^64 - 1)`): tests/test_rng_host.py checks the layout's
stream hygiene on the host, tests/test_gpu_rng.py holds every consumer's own draws to it on the device.
"""
import numpy as np

M64 = (1 << 64) - 1
U64 = np.uint64

# ------------------------------------------------------------------------------------------------ constants of the C side
STREAM_MUL = 0xD6E8FEB86659FD93      # sg_key: seed ^ stream * STREAM_MUL
ROUND_MUL = 0x632BE59BD9B4E019       # sg_feistel: key + round * ROUND_MUL + r
PERM_STREAM = 0x5045524D             # sg_fill_perm: key = sg_key(seed, PERM_STREAM, stream_id)
SG_ACT_STREAM = 0x41435400           # sg_policy_fwd.hpp
SG_KFAC_STREAM = 0xACC7000000        # sg_kfac.hpp
PPO_EPOCH_MUL = 2654435761           # sg_ppo.hip: stream_id = e * PPO_EPOCH_MUL (+ rank)
DISC_EPERM_STREAM = 0xE0000000       # sg_disc.hip: + rng_calls
DISC_PPERM_STREAM = 0xF0000000       # + rng_calls * 1024 + rank (sharded mode; 0 otherwise)
DISC_ALPHA_STREAM = 0xA1000000       # + rng_calls
GRAD_PEN_STREAM = 0xA2000000         # sg_disc_grad_pen
TWO_PI_F32 = float(np.float32(6.28318530717958647692))   # the constant sg_normal multiplies u2 by, as float32 holds it
# simgan_amd/utils.py: derive_seed's salts
SALT_POLICY, SALT_ENSEMBLE, SALT_PPO, SALT_ACKTR, SALT_DISC = 0x5EED, 0xE5E, 0xBADC0FFEE, 0xACC7, 0xD15C


def u64(x):
    """ints (any size: reduced modulo 2^64) / arrays -> uint64 array of at least one dimension."""
    if isinstance(x, np.ndarray) and x.dtype == U64:
        return np.atleast_1d(x)
    if isinstance(x, np.ndarray):
        return np.atleast_1d(x.astype(U64))
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & M64 for v in x], dtype=U64)
    return np.array([int(x) & M64], dtype=U64)


# ------------------------------------------------------------------------------------------------ the generator, exact
def mix64(x):
    """sg_mix64: the splitmix64 step (add the golden-ratio increment, then the finaliser)."""
    x = u64(x) + U64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def mix64_int(x):
    """sg_mix64 on one Python int: the same function without numpy, for cross-checks."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def stream_key(seed, stream):
    """The first level of sg_key: sg_mix64(seed ^ stream * STREAM_MUL).  A stream's draws are sg_mix64(stream_key + counter)."""
    return mix64(u64(seed) ^ (u64(stream) * U64(STREAM_MUL)))


def key(seed, stream, ctr):
    """sg_key(seed, stream, ctr)"""
    return mix64(stream_key(seed, stream) + u64(ctr))


def uniform(seed, stream, ctr):
    """sg_uniform: the key's top 24 bits / 2^24, float32 (exact: both the integer and the scaled value are representable)."""
    return ((key(seed, stream, ctr) >> U64(40)).astype(np.float64) / 16777216.0).astype(np.float32)


def normal_uniforms(seed, stream, ctr):
    """(u1, u2) of sg_normal as float64 (both exact in float32 too): u1 = (top 24 bits + 1) / 2^24 in (0, 1], u2 = bits 16..39 / 2^24."""
    k = key(seed, stream, ctr)
    u1 = ((k >> U64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((k >> U64(16)) & U64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return u1, u2


def normal64(seed, stream, ctr):
    """sg_normal's Box-Muller in float64, from the same key, the same u1 / u2 and the float32 value of the 2 pi constant."""
    u1, u2 = normal_uniforms(seed, stream, ctr)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


def normal32(seed, stream, ctr):
    """The same formula with every operation in numpy float32, operation for operation as sg_normal writes it (numpy's libm):
    its distance from normal64 is what float32 arithmetic costs this formula."""
    u1, u2 = normal_uniforms(seed, stream, ctr)
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(TWO_PI_F32) * u2)


def find_u1_ends(seed, stream, limit=1 << 31, chunk=1 << 22):
    """The first counters of (seed, stream) at which sg_normal's u1 is 2^-24 (the key's top 24 bits all zero: the largest
    |z| the generator can give) and 1 (all ones: log u1 = 0), found by scanning -- about 2^24 counters each."""
    lo = hi = None
    for c in range(0, limit, chunk):
        top = key(seed, stream, np.arange(c, c + chunk, dtype=U64)) >> U64(40)
        if lo is None and (top == U64(0)).any():
            lo = c + int(np.argmax(top == U64(0)))
        if hi is None and (top == U64(0xFFFFFF)).any():
            hi = c + int(np.argmax(top == U64(0xFFFFFF)))
        if lo is not None and hi is not None:
            return lo, hi
    raise AssertionError(f"no counter below {limit} reaches both ends of u1")


def perm_half_bits(n):
    """sg_perm_half_bits: the smallest hb >= 1 with 2^(2 hb) >= n."""
    hb = 1
    while (1 << (2 * hb)) < n:
        hb += 1
    return hb


def feistel(x, half_bits, k):
    """sg_feistel: six rounds of a balanced Feistel network on 2 * half_bits bits; x uint array, k one uint64 key."""
    x = u64(x)
    k = int(u64(k)[0])
    mask = U64((1 << half_bits) - 1)
    l, r = x >> U64(half_bits), x & mask
    for rnd in range(6):
        f = (mix64(U64((k + rnd * ROUND_MUL) & M64) + r) >> U64(32)) & mask
        l, r = r, l ^ f
    return (l << U64(half_bits)) | r


def perm_at(i, n, half_bits, k):
    """sg_perm_at: walk the Feistel cycle from i until the value falls inside [0, n)."""
    x = feistel(u64(i), half_bits, k)
    out = x >= U64(n)
    while out.any():
        x[out] = feistel(x[out], half_bits, k)
        out = x >= U64(n)
    return x.astype(np.int64)


def first_hits(n, k):
    """How many i in [0, n) land inside [0, n) at the first Feistel application (no cycle walking)."""
    return int((feistel(np.arange(n, dtype=U64), perm_half_bits(n), k) < U64(n)).sum())


def perm_key(seed, stream_id):
    """The key sg_fill_perm draws a permutation under: the stream is PERM_STREAM, the caller's stream id is the COUNTER."""
    return key(seed, PERM_STREAM, stream_id)


def fill_perm(n, seed, stream_id):
    """sg_fill_perm: the permutation of [0, n) under (seed, stream_id) -> int64 [n]."""
    return perm_at(np.arange(n, dtype=U64), n, perm_half_bits(n), perm_key(seed, stream_id))


# ------------------------------------------------------------------------------------------------ the Python side's seeds
def derive_seed(seed, salt, inst=0):
    """simgan_amd.utils.derive_seed with the per-process instance number as an argument (0: not per instance)."""
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(salt) * STREAM_MUL + int(inst) * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 2


def call_seed(obj_seed, calls):
    """The seed an object hands the library on its calls-th stochastic call (calls counted from 1: incremented before use)."""
    return (int(obj_seed) + int(calls)) & M64


# ------------------------------------------------------------------------------------------------ the consumers' layouts
# Each returns (seed, stream, counters): element [..] of the consumer's draw array is the generator at counters[..].
def act_layout(obj_seed, call, rank, n, width):
    """Action draws of one act call over n rows: counter row * width + j on stream SG_ACT_STREAM + rank, seed obj.seed + call.
    width: A (Gaussian, standard normals), the number of bits (Bernoulli, uniforms), 1 (Categorical: one uniform per row).
    `row` is the row of the batch the call was given, whatever tile, pass, ensemble member or launch form computes it.
    Policy.act, act_rnn, PolicyEnsemble.act (obj = the ensemble), RolloutStorage.act_step / act_step_rnn (obj = the policy) and
    both halves of act_step_chain (learner: the policy's seed and calls; inner: the ensemble's) all draw this way."""
    ctr = np.arange(n * width, dtype=U64).reshape(n, width)
    return call_seed(obj_seed, call), SG_ACT_STREAM + rank, ctr


def ppo_perm_layout(obj_seed, call, epoch, rank=0):
    """(seed, stream_id) of PPO's minibatch permutation of epoch `epoch` in its call-th update.  rank: the feed-forward
    data-parallel update adds it; the recurrent and the CNN update run on one rank (rank 0)."""
    return call_seed(obj_seed, call), (epoch * PPO_EPOCH_MUL + rank) & M64


def ppo_perms(obj_seed, call, epochs, n, rank=0):
    """[epochs, n] as agent.last_perms() returns them after the call-th update without perms=."""
    return np.stack([fill_perm(n, *ppo_perm_layout(obj_seed, call, e, rank)) for e in range(epochs)])


def disc_layout(obj_seed, call, rng_call, rank=0, sharded=False):
    """The D step's three draws in the object's call-th stochastic call (update epochs and grad-pen calls both count) that is
    the handle's rng_call-th update epoch: {"eperm": (seed, stream_id), "pperm": (seed, stream_id), "alpha": (seed, stream)}.
    The expert permutation and alpha are the same on every rank; the policy permutation adds the rank in sharded mode."""
    s = call_seed(obj_seed, call)
    return {"eperm": (s, DISC_EPERM_STREAM + rng_call),
            "pperm": (s, DISC_PPERM_STREAM + rng_call * 1024 + (rank if sharded else 0)),
            "alpha": (s, DISC_ALPHA_STREAM + rng_call)}


def disc_draws(obj_seed, call, rng_call, n_expert, tn, n_alpha, rank=0, sharded=False):
    """(eperm, pperm, alpha) as D.last_draws() returns them."""
    lay = disc_layout(obj_seed, call, rng_call, rank, sharded)
    return (fill_perm(n_expert, *lay["eperm"]), fill_perm(tn, *lay["pperm"]),
            uniform(*lay["alpha"], np.arange(n_alpha, dtype=U64)))


def grad_pen_layout(obj_seed, call, n):
    """compute_grad_pen's alpha: n uniforms on GRAD_PEN_STREAM."""
    return call_seed(obj_seed, call), GRAD_PEN_STREAM, np.arange(n, dtype=U64)


def acktr_layout(obj_seed, update, tn):
    """ACKTR's value noise of update `update` (counted from 0): the object's seed itself, stream SG_KFAC_STREAM + update."""
    return int(obj_seed) & M64, SG_KFAC_STREAM + update, np.arange(tn, dtype=U64)
