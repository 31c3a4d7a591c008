"""The numpy restatement of the dropout generator (rowwise_ref.dropout_mask) on its own: the GPU tests compare kernels with it
bit for bit, so it must itself behave like a Bernoulli(1 - thr/65536) mask for every (seed, n, p) they use."""
import math

import numpy as np
import pytest

import rowwise_ref as R


@pytest.mark.parametrize("seed,n,p", R.MASK_CASES)
def test_keep_fraction_within_four_sigma(seed, n, p):
    q = 1.0 - R.dropout_threshold(p) / 65536.0
    kept = R.dropout_mask(seed, 0, n, p)
    assert kept.dtype == np.bool_ and kept.shape == (n,)
    sigma = math.sqrt(q * (1.0 - q) / n)
    assert abs(kept.mean() - q) <= 4.0 * sigma, (kept.mean(), q, sigma)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_high_seed_word_changes_the_mask(p):
    """seeds that differ only in their high word give independent masks: they agree where both keep or both drop.  (A small seed
    only permutes the pair index through the XOR; the high word enters between the two multiply rounds.)
    The high words must differ in many bits, as those of ops.next_seed() do (its output is multiplied and folded): a single
    multiply round follows the high word, so high words 5 and 6 give masks that agree on 25 % of the elements at p = 0.5, not
    50 % -- a property of the generator as specified, which its callers never meet."""
    n = 524608
    q = 1.0 - R.dropout_threshold(p) / 65536.0
    agree = q * q + (1.0 - q) * (1.0 - q)
    sigma = math.sqrt(agree * (1.0 - agree) / n)
    for s1, s2 in ((R.SEED_HI, (0x9E3779B9 << 32) | 17), (R.SEED_HI, R.EMBED_SEED)):
        a, b = R.dropout_mask(s1, 0, n, p), R.dropout_mask(s2, 0, n, p)
        assert abs((a == b).mean() - agree) <= 4.0 * sigma
    # ... while the low word of a small seed is a permutation of pairs: seed 0 at pair k is seed 77 at pair k ^ 77
    c, d = R.dropout_mask(0, 0, 512, p), R.dropout_mask(77, 0, 512, p)
    k = np.arange(512)
    assert np.array_equal(c, d[(((k >> 1) ^ 77) << 1) | (k & 1)])


def test_mask_is_a_function_of_the_absolute_index():
    full = R.dropout_mask(R.SEED_HI, 0, 5000, 0.3)
    for start in (1, 2, 255, 1027):
        assert np.array_equal(R.dropout_mask(R.SEED_HI, start, 300, 0.3), full[start:start + 300])
    # indices past 2^32 use the high half of the pair index (rotl(hi, 7)): they differ from the low ones
    far = R.dropout_mask(R.SEED_HI, (1 << 33), 4096, 0.3)
    assert not np.array_equal(far, full[:4096])


def test_threshold_and_extremes():
    assert R.dropout_threshold(0.0) == 0 and R.dropout_threshold(0.5) == 32768
    assert R.dropout_threshold(0.1) == 6554 and R.dropout_threshold(0.25) == 16384
    assert R.dropout_mask(R.SEED_LO, 0, 1000, 0.0).all()
    # the two halves of one hash decide an even element and its odd neighbour
    h = R._hash32(R.SEED_HI, np.arange(8, dtype=np.uint64))
    thr = R.dropout_threshold(0.3)
    m = R.dropout_mask(R.SEED_HI, 0, 16, 0.3)
    assert np.array_equal(m[0::2], (h & np.uint64(0xFFFF)) >= thr) and np.array_equal(m[1::2], (h >> np.uint64(16)) >= thr)
