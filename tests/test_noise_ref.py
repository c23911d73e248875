"""The numpy restatement of the device's normal stream (tests/noise_ref.py) on its own, without a GPU: the block function
against Random123's published known-answer vectors, and the statistical thresholds the GPU test applies to the device's
output (tests/test_gpu_noise_draws.py) on the same fixed keys — so they are known to be passable before a GPU is involved."""
import numpy as np
import pytest

import noise_ref as R


def test_block_function_is_philox4x32_10():
    """Random123's kat_vectors for philox4x32-10: counter and key passed through directly."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in R.philox4x32(ctr, key)) == want


def test_stream_layout():
    """Pairs: sample 2q and 2q + 1 come from block q; a prefix of a note's stream is the stream of a shorter note; tags, ids and
    seeds select different streams; seed and id enter through their XOR only."""
    z = R.normals(11, 5, 0, 1001)
    assert z.dtype == np.float64 and z.shape == (1001,) and np.isfinite(z).all()
    assert np.array_equal(R.normals(11, 5, 0, 7), z[:7]) and np.array_equal(R.normals(11, 5, 0, 1), z[:1])
    assert np.array_equal(R.normals(11 ^ 5, 0, 0, 1001), z)
    for other in (R.normals(11, 5, 1, 1001), R.normals(11, 6, 0, 1001), R.normals(12, 5, 0, 1001), R.normals(11, 5 + (1 << 32), 0, 1001)):
        assert not np.any(other == z)
    # r^2 = -2 ln u1 and the angle are shared by the two samples of a pair
    r2 = z[0:1000:2] ** 2 + z[1:1000:2] ** 2
    assert (r2 >= 0).all() and r2.max() <= -2.0 * np.log(2.0 ** -53) + 1e-9
    g = R.growl(11, 5, 1001, 0.3)
    assert np.allclose(np.log2(2.0 * g), 0.09 * R.normals(11, 5, 4, 1001), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", range(len(R.STAT_KEYS)))
def test_restatement_passes_the_thresholds(case):
    seed, note = R.STAT_KEYS[case]
    tag = case % 5
    z = R.normals(seed, note, tag, R.STAT_N)
    R.assert_normal(z, f"key {case} tag {tag}")
    c = R.correlation(z, R.normals(seed, note, (tag + 1) % 5, R.STAT_N))
    print("cross-stream", round(c, 3))
    assert c < R.SE_MAX
    c = R.correlation(z, R.normals(seed, note + 1, tag, R.STAT_N))     # two notes that differ only in id
    print("cross-note", round(c, 3))
    assert c < R.SE_MAX
