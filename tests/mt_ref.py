"""numpy's legacy normal stream (``np.random.seed(s); np.random.randn(n)``) restated in plain integer / float64 arithmetic: the
definition goofer_legacy_normal_fill documents (include/goofer_hip.h) and k_legacy_normal_fill implements.

  seeding   mt[0] = s, mt[i] = (1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i) mod 2^32; position 624, no cached normal
  block     624 words twisted in place in index order (twist_sequential), or in the three wide steps the kernel takes
            (twist_parallel), then tempered as they are drawn
  double    two words a, b: ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0
  attempt   two doubles: x1 = 2 d0 - 1, x2 = 2 d1 - 1, r2 = x1 x1 + x2 x2; rejected when r2 >= 1 or r2 == 0; else
            f = sqrt(-2 log(r2) / r2) and the normals f x2, f x1 in that order
A block is 156 whole attempts.  ``log`` is the C library's (math.log), as in numpy's legacy_gauss."""
import math

import numpy as np

WORDS, SHIFT, ATTEMPTS = 624, 397, 156
MASK32 = 0xFFFFFFFF


def seed_words(seed):
    """the 624 state words ``np.random.seed(seed)`` leaves (uint32)"""
    mt = [int(seed) & MASK32]
    for i in range(1, WORDS):
        mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & MASK32)
    return np.array(mt, dtype=np.uint32)


def twist_sequential(mt):
    """the next block's state words: k = 0..623 in order and in place"""
    mt = [int(v) for v in mt]
    for k in range(WORDS):
        y = (mt[k] & 0x80000000) | (mt[(k + 1) % WORDS] & 0x7FFFFFFF)
        mt[k] = mt[(k + SHIFT) % WORDS] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
    return np.array(mt, dtype=np.uint32)


def twist_parallel(mt):
    """the same in three wide steps: [0, 227) reads old words only, [227, 454) the new words of [0, 227), [454, 624) the new
    words of [227, 397) and (k = 623) the new mt[0]; each step reads all its operands before it writes"""
    mt = np.array(mt, dtype=np.uint32)
    for lo, hi in ((0, 227), (227, 454), (454, 624)):
        k = np.arange(lo, hi)
        y = (mt[k] & np.uint32(0x80000000)) | (mt[(k + 1) % WORDS] & np.uint32(0x7FFFFFFF))
        new = mt[(k + SHIFT) % WORDS] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908B0DF), np.uint32(0))
        mt[k] = new
    return mt


def temper(y):
    y = np.array(y, dtype=np.uint32)
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xEFC60000))
    return y ^ (y >> np.uint32(18))


def block_attempts(mt):
    """(accepted [156] bool, first normal, second normal) of the 156 attempts of a block whose (untempered) state is ``mt``"""
    w = temper(mt).astype(np.uint64).reshape(-1, 2)
    d = ((w[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[:, 1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
    d = d.reshape(-1, 2)
    x1, x2 = 2.0 * d[:, 0] - 1.0, 2.0 * d[:, 1] - 1.0
    r2 = x1 * x1 + x2 * x2
    acc = ~((r2 >= 1.0) | (r2 == 0.0))
    f = np.zeros(ATTEMPTS)
    f[acc] = [math.sqrt(-2.0 * math.log(v) / v) for v in r2[acc].tolist()]
    return acc, f * x2, f * x1


def draw(seed, m, twist=twist_parallel):
    """The first ``m`` normals after ``np.random.seed(seed)`` and what the generator looks like afterwards:
    (normals [m], attempts made, state) with state = (key [624] uint32, position, has_gauss, cached normal) as
    ``np.random.get_state()`` reports it."""
    mt = seed_words(seed)
    out, have, attempts, blocks = [], 0, 0, 0
    pos, cached = WORDS, 0.0
    need = (m + 1) // 2                                        # accepted attempts
    while have < need:
        mt = twist(mt)
        blocks += 1
        acc, a, b = block_attempts(mt)
        idx = np.nonzero(acc)[0]
        take = min(idx.size, need - have)
        idx = idx[:take]
        out.append(np.stack([a[idx], b[idx]], axis=1).reshape(-1))
        have += take
        last = int(idx[-1]) + 1 if take else 0                 # attempts of this block the draws consumed
        attempts = (blocks - 1) * ATTEMPTS + last
        pos = 4 * last
    z = np.concatenate(out) if out else np.zeros(0)
    has_gauss = int(m % 2 == 1)
    if has_gauss:
        cached = float(z[m])
    return z[:m], attempts, (mt, pos, has_gauss, cached)


def expected_blocks(m):
    """ceil(m / (2 * 156 * pi / 4)): the blocks m normals take on average"""
    return int(math.ceil(m / (2.0 * ATTEMPTS * math.pi / 4.0)))
