"""CPU: bbgr.text.plan_group_ranges, the host planner of the regrouped pooled
count, against a brute-force restatement of its rule on random prefixes, at
its edges, and on the committed corpus of tests/test_gpu_features_v2.py."""
import numpy as np
import pytest

import features_v2_ref as V
from bbgr.text import BYTES_MAX, plan_chunks, plan_group_ranges


def _brute(sizes, chunk_bytes):
    """Group after group: a range takes groups while their bytes fit; its
    first group always goes in."""
    out, g0, G = [], 0, len(sizes)
    while g0 < G:
        g1, have = g0 + 1, int(sizes[g0])
        while g1 < G and have + int(sizes[g1]) <= chunk_bytes:
            have += int(sizes[g1])
            g1 += 1
        out.append((g0, g1))
        g0 = g1
    return out


def _prefix(sizes):
    p = np.zeros(len(sizes) + 1, np.int64)
    if len(sizes):
        np.cumsum(np.asarray(sizes, np.int64), out=p[1:])
    return p


def _check(sizes, chunk_bytes):
    got = plan_group_ranges(_prefix(sizes), chunk_bytes)
    assert got == _brute(sizes, chunk_bytes), (list(sizes), chunk_bytes)
    # consecutive, covering [0, G), and only a group of its own may exceed the chunk
    assert [a for a, _ in got] == [0] * bool(got) + [b for _, b in got[:-1]]
    assert (got[-1][1] if got else 0) == len(sizes)
    for g0, g1 in got:
        assert g1 > g0
        assert g1 - g0 == 1 or int(np.sum(sizes[g0:g1])) <= chunk_bytes
    return got


@pytest.mark.parametrize("seed", range(8))
def test_random_prefixes_against_the_restatement(seed):
    rng = np.random.default_rng(seed)
    G = int(rng.integers(1, 200))
    sizes = rng.integers(0, 5000, G)
    sizes[rng.uniform(size=G) < 0.3] = 0                     # empty groups anywhere
    if seed % 2:
        sizes[:3], sizes[-4:] = 0, 0                         # leading and trailing ones
    if not sizes.any():
        sizes[G // 2] = 17
    largest, total = int(sizes.max()), int(sizes.sum())
    for c in (1, largest - 1, largest, total, total + 1, 777, 1 << 40):
        if c >= 1:
            _check(sizes, c)


def test_edges():
    assert plan_group_ranges(np.zeros(1, np.int64), 10) == []          # G = 0
    assert plan_group_ranges(_prefix([0]), 1) == [(0, 1)]              # G = 1, empty
    assert plan_group_ranges(_prefix([99]), 1) == [(0, 1)]             # G = 1, larger than the chunk
    assert _check(np.asarray([0, 0, 0]), 1) == [(0, 3)]                # only empty groups
    assert _check(np.asarray([0, 0, 5, 0, 0, 5, 0]), 5) == [(0, 5), (5, 7)]
    # a group over the chunk runs alone: the empty ones behind it open the next range
    assert _check(np.asarray([0, 0, 5, 0, 0, 5, 0]), 4) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 7)]
    assert _check(np.asarray([3, 3, 3, 3]), 6) == [(0, 2), (2, 4)]
    assert _check(np.asarray([3, 3, 3, 3]), 12) == [(0, 4)]


def test_the_rule_is_plan_chunks_over_groups():
    rng = np.random.default_rng(11)
    p = _prefix(rng.integers(0, 300, 500))
    for c in (1, 100, 299, 300, 5000):
        assert plan_group_ranges(p, c) == plan_chunks(p, c)


def test_value_errors():
    p = _prefix([5, 6, 7])
    for bad in (0, -1):
        with pytest.raises(ValueError, match="chunk_bytes"):
            plan_group_ranges(p, bad)
    with pytest.raises(ValueError, match=rf"group 1 has {BYTES_MAX} bytes"):
        plan_group_ranges(_prefix([5, BYTES_MAX, 7]), 1 << 20)
    # one byte less is taken, alone, whatever chunk_bytes says: it is capped below 2^31 - 1
    assert plan_group_ranges(_prefix([5, BYTES_MAX - 1, 7]), 1 << 40) == [(0, 1), (1, 2), (2, 3)]
    assert plan_group_ranges(_prefix([5, BYTES_MAX - 6, 1]), 1 << 40) == [(0, 2), (2, 3)]


def test_the_committed_corpus():
    corpus = V.gpu_corpus()
    _, offsets = V.text_of(corpus["records"])
    sizes = np.bincount(corpus["user"], weights=np.diff(offsets), minlength=V.U).astype(np.int64)
    assert (len(corpus["records"]), int(offsets[-1]), sizes.size) == (19_636, 2_446_393, 300)
    assert int(sizes[0]) == 588_553 and int(np.sort(sizes)[-2]) == 10_961
    counts = [len(_check(sizes, c)) for c in (1, 4096, 65536, 1 << 20)]
    assert counts == [300, 296, 31, 3]
