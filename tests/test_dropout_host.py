"""The dropout mask contract (ndcn_amd/csrc/dropout.h) on the host: the numpy reference of tests/_philox.py against Philox4x32-10's
known answers, the statistics of the masks it defines, and the stream module that hands out (seed, evaluation) - ndcn_amd/dropout.py.
The kernels are compared with the same reference bit for bit in tests/test_gpu_dropout.py."""
import numpy as np
import pytest
import torch

import _philox

SEED = 0x0000567800001234


def test_philox_known_answers():
    got = [int(x) for x in _philox.philox4x32_10([0, 0, 0, 0], (0, 0))]
    assert got == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = [int(x) for x in _philox.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0))]
    assert got == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_words_do_not_depend_on_where_the_range_starts():
    full = _philox.words(SEED, 3, 1000)
    for first, n in ((0, 1), (1, 7), (3, 5), (4, 4), (997, 3)):
        assert np.array_equal(_philox.words(SEED, 3, n, first=first), full[first:first + n])
    # element indices past 2^32 groups reach the second counter word
    big = _philox.words(SEED, 3, 8, first=(1 << 34) + 4)
    assert not np.array_equal(big, _philox.words(SEED, 3, 8, first=4))


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_keep_rate(p):
    n = 1 << 22
    rate = float(_philox.kept(p, SEED, 7, n).mean())
    sigma = np.sqrt(p * (1 - p) / n)
    print('p = %.1f: keep rate %.6f, %.2f standard deviations from 1 - p' % (p, rate, abs(rate - (1 - p)) / sigma))
    assert abs(rate - (1 - p)) <= 5 * sigma


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_masks_of_neighbouring_evaluations_and_seeds_are_independent(p):
    n = 1 << 22
    base = _philox.kept(p, SEED, 7, n)
    expect = p * p + (1 - p) * (1 - p)                     # two independent Bernoulli masks agree with this probability
    sigma = np.sqrt(expect * (1 - expect) / n)
    for other in (_philox.kept(p, SEED, 8, n), _philox.kept(p, SEED + 1, 7, n)):
        share = float((base == other).mean())
        assert abs(share - expect) <= 5 * sigma, (share, expect, sigma)


def test_mask_values_and_scale():
    m = _philox.mask(0.5, SEED, 0, 64, 20)
    assert m.dtype == np.float32 and m.shape == (64, 20)
    assert set(np.unique(m).tolist()) == {0.0, 2.0}
    s = _philox.scale(0.1)
    assert s.dtype == np.float32 and s == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1))
    assert _philox.threshold(0.5) == 1 << 31 and 0 < _philox.threshold(0.9) < 1 << 32


def test_stream_seeds_repeat_under_manual_seed_and_counters_start_at_zero_per_solve():
    from ndcn_amd import dropout

    def run():
        torch.manual_seed(3)
        out = []
        for _ in range(3):
            with dropout.solve_scope():
                out.append([dropout.next_evaluation(0.5) for _ in range(4)])
        out.append(dropout.next_evaluation(0.25))               # outside a solve: a stream of its own
        return out
    a, b = run(), run()
    assert a == b
    for solve in a[:3]:
        assert [e for _, _, e in solve] == [0, 1, 2, 3]
        assert len({s for _, s, _ in solve}) == 1 and 0 <= solve[0][1] < 2 ** 64
    seeds = [solve[0][1] for solve in a[:3]] + [a[3][1]]
    assert len(set(seeds)) == 4
    assert a[3][0] == 0.25 and a[3][2] == 0
    torch.manual_seed(4)
    with dropout.solve_scope():
        assert dropout.next_evaluation(0.5)[1] != a[0][0][1]


def test_a_solve_without_active_dropout_leaves_the_generator_alone():
    from ndcn_amd import dropout
    torch.manual_seed(5)
    want = torch.rand(3)
    torch.manual_seed(5)
    with dropout.solve_scope() as stream:
        assert stream.take(6) == 0 and stream.take() == 6      # counters alone draw nothing
    assert torch.equal(torch.rand(3), want)


def test_scopes_nest_and_blocks_of_counters_do_not_overlap():
    from ndcn_amd import dropout
    assert dropout.current() is None
    with dropout.solve_scope() as outer:
        first = outer.take(8)
        with dropout.solve_scope() as inner:
            assert dropout.current() is inner and dropout.next_evaluation(0.5)[2] == 0
        assert dropout.current() is outer
        assert (first, dropout.next_evaluation(0.5)[2]) == (0, 8)
    assert dropout.current() is None


def test_is_active_and_scale():
    from ndcn_amd import dropout

    class M:
        def __init__(self, p, training):
            self.dropout, self.training = p, training
    assert dropout.is_active(M(0.5, True)) and not dropout.is_active(M(0.5, False))
    assert not dropout.is_active(M(0.0, True)) and not dropout.is_active(M(1.0, True))
    assert dropout.scale(0.5) == 2.0 and dropout.scale(0.1) == float(_philox.scale(0.1))
