"""goofer_legacy_normal_jobs restated in numpy on top of tests/mt_ref.py: the job rule (include/goofer_hip.h).

  job      (seed, n, destinations, f32): the first n * len(destinations) normals after ``np.random.seed(seed)``; normal p goes
           to destination p // n at sample p % n — one ``np.random.randn(n)`` per destination, in order, the polar method's
           second value carried from one to the next
  null     a destination that is None consumes its n draws and stores nothing
  empty    n == 0 or no destination: nothing is drawn, 0 attempts
  f32      every normal rounded to float32 and widened again (``randn(n).astype(np.float32).astype(np.float64)``)"""
import numpy as np

import mt_ref


def job(seed, n, n_dst, f32=False):
    """(normals [n_dst, n] float64, attempts) of one job with ``n_dst`` destinations"""
    m = n * n_dst if n > 0 else 0
    if m == 0:
        return np.zeros((n_dst, max(n, 0))), 0
    z, attempts, _ = mt_ref.draw(seed, m)
    if f32:
        z = z.astype(np.float32).astype(np.float64)
    return z.reshape(n_dst, n), attempts


def run(table, arrays):
    """A job table on host arrays: ``table`` rows (seed, n, [(name, offset) or None, ...], f32), ``arrays`` {name: float64
    array}, written in place where a job stores.  Returns the jobs' attempts (int64)."""
    attempts = np.zeros(len(table), dtype=np.int64)
    for j, (seed, n, dsts, f32) in enumerate(table):
        z, attempts[j] = job(seed, n, len(dsts), f32)
        for k, d in enumerate(dsts):
            if d is not None:
                name, off = d
                arrays[name][off:off + n] = z[k]
    return attempts
