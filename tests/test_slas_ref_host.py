"""CPU: the host restatement of the SLAS sampler's keys (tests/slas_ref.py),
checked on its own before the GPU tests rely on it: Philox4x32-10 against the
Random123 known-answer vectors, the counter / key layout of slas_u24 against a
scalar pure-Python restatement, and the power of check_picks."""
import numpy as np
import pytest

import slas_ref as SR

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = SR.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want
    # vectorised: the same words at every position of an array of counters
    arr = SR.philox4x32_10(*(np.full(5, c, np.uint64) for c in ctr), *key)
    for a, w in zip(arr, want):
        assert a.shape == (5,) and (a == w).all()


def _philox_scalar(c, k):
    """Philox4x32-10 with Python integers, one counter."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_scalar_restatement_meets_the_vectors():
    for ctr, key, want in KAT:
        assert tuple(_philox_scalar(ctr, key)) == want


def test_u24_layout_against_scalar():
    seed, counter, stage, row = (0x9E3779B9 << 32) | 0x7F4A7C15, 2 ** 31 + 12345, 255, 70001
    assert seed > 2 ** 32
    pos = np.array([0, 1, 63, 64, 1024, 19999, 2 ** 24 + 3], np.int64)
    got = SR.slas_u24(seed, counter, stage, row, pos)
    want = [(_philox_scalar((counter, stage, row, int(p)), (seed & 0xFFFFFFFF, seed >> 32))[0] >> 8)
            + 1 for p in pos]
    assert got.dtype == np.int64 and got.tolist() == want
    assert ((got >= 1) & (got <= 2 ** 24)).all()
    # a per-slot row array gives what the scalar row gives
    assert SR.slas_u24(seed, counter, stage, np.full(pos.size, row), pos).tolist() == want
    # every word matters: high seed word, counter bit 31, stage, row, position
    for other in (SR.slas_u24(seed & 0xFFFFFFFF, counter, stage, row, pos),
                  SR.slas_u24(seed, counter - 2 ** 31, stage, row, pos),
                  SR.slas_u24(seed, counter, 254, row, pos),
                  SR.slas_u24(seed, counter, stage, row + 1, pos),
                  SR.slas_u24(seed, counter, stage, row, pos + 1)):
        assert (other != got).all()


def test_keys_and_weights():
    u24 = np.array([2 ** 24, 2 ** 23, 1, 2 ** 22])
    w = SR.slas_weights64(np.array([0.0, 0.5, -0.5, 1.0]), 2.0, labels=np.array([1, -1, 0, -1]),
                          upweight=1.0)
    np.testing.assert_allclose(w, [2.0, np.e, 2.0 / np.e, np.e ** 2], rtol=1e-15)
    keys = SR.slas_keys64(u24, w, np.array([True, True, True, False]))
    np.testing.assert_allclose(keys[:3], [0.0, np.log(2) / np.e, 24 * np.log(2) * np.e / 2.0],
                               rtol=1e-15)
    assert keys[3] == np.inf and not np.signbit(keys[0])
    # the clamp, and NaN as fminf(fmaxf(.)) leaves it
    w = SR.slas_weights64(np.array([1.0, -1.0, np.nan, np.inf, -np.inf]), 200.0)
    assert w.tolist() == [SR.FLT_MAX, SR.FLT_MIN, SR.FLT_MIN, SR.FLT_MAX, SR.FLT_MIN]
    row, pos = SR.slot_rows([0, 2, 2, 5])
    assert row.tolist() == [0, 0, 2, 2, 2] and pos.tolist() == [0, 1, 0, 1, 2]


def test_delta_is_the_written_budget():
    assert SR.key_error_budget(2, 3.0) == (9 + 18) * 2.0 ** -24
    assert SR.pick_delta(2, 3.0) == 4 * 27 * 2.0 ** -24          # 6.4e-6
    assert SR.pick_delta(16, 3.0) == 4 * 69 * 2.0 ** -24         # 1.6e-5
    assert SR.pick_delta(2, 0.0) == 4 * 18 * 2.0 ** -24


# -- check_picks has power ---------------------------------------------------------
K, DELTA = 15, SR.pick_delta(2, 3.0)


def _row():
    """300 slots, 40 of them ineligible, weights over exp(+-3), one exact tie
    (u24 and w) between the picks 4 and 5; every other gap in the first K + 1
    keys is far above DELTA."""
    rng = np.random.default_rng(7)
    m = 300
    u24 = SR.slas_u24(42, 5, 0, 3, np.arange(m))
    w = SR.slas_weights64(rng.uniform(-1, 1, m), 3.0)
    eligible = np.ones(m, bool)
    eligible[rng.permutation(m)[:40]] = False
    order = np.argsort(SR.slas_keys64(u24, w, eligible), kind="stable")
    a, b = sorted(order[4:6].tolist())
    u24[b], w[b] = u24[a], w[a]
    keys = SR.slas_keys64(u24, w, eligible)
    order = np.lexsort((np.arange(m), keys))
    assert sorted(order[4:6].tolist()) == [a, b] and keys[a] == keys[b]
    top = keys[order[:K + 1]]
    gaps = 1.0 - top[:-1] / top[1:]
    assert (np.delete(gaps, 4) > 100 * DELTA).all()
    return keys, eligible, u24, w, order


def test_check_picks_accepts_the_argsort():
    keys, eligible, u24, w, order = _row()
    assert SR.check_picks(keys, eligible, order[:K], DELTA, u24, w) == 0.0
    assert SR.check_picks(keys, eligible, order[:1], DELTA, u24, w) == 0.0
    # an inversion inside delta is accepted and reported
    k2 = keys.copy()
    k2[order[9]] = k2[order[8]] * (1 - DELTA / 2)
    inv = SR.check_picks(k2, eligible, order[:K], DELTA, u24, w)
    assert 0.4 * DELTA < inv < 0.6 * DELTA
    # all eligible slots picked: nothing is left to beat the last pick
    few = np.zeros(keys.size, bool)
    few[order[:K]] = True
    assert SR.check_picks(keys, few, order[:K], DELTA, u24, w) == 0.0


def _rejected(keys, eligible, picks, u24, w, what):
    with pytest.raises(AssertionError, match=what):
        SR.check_picks(keys, eligible, picks, DELTA, u24, w)


def test_check_picks_rejects_the_next_slot():
    keys, eligible, u24, w, order = _row()
    for j in (0, 7, K - 1):
        picks = order[:K].copy()
        picks[j] = order[K]
        picks = picks[np.argsort(keys[picks], kind="stable")]     # still ascending
        _rejected(keys, eligible, picks, u24, w, "unpicked slot beats")


def test_check_picks_rejects_a_swap():
    keys, eligible, u24, w, order = _row()
    for j in (0, 8, K - 2):
        picks = order[:K].copy()
        picks[[j, j + 1]] = picks[[j + 1, j]]
        _rejected(keys, eligible, picks, u24, w, "ascending key order")


def test_check_picks_rejects_a_tie_written_higher_slot_first():
    keys, eligible, u24, w, order = _row()
    picks = order[:K].copy()
    picks[[4, 5]] = picks[[5, 4]]
    _rejected(keys, eligible, picks, u24, w, "higher slot first")
    # without u24 / w the tie cannot be judged: the keys alone are equal
    SR.check_picks(keys, eligible, picks, DELTA)


def test_check_picks_rejects_an_ineligible_slot():
    keys, eligible, u24, w, order = _row()
    picks = order[:K].copy()
    picks[3] = np.flatnonzero(~eligible)[0]
    _rejected(keys, eligible, picks, u24, w, "ineligible")


def test_check_picks_rejects_a_repeated_slot():
    keys, eligible, u24, w, order = _row()
    picks = order[:K].copy()
    picks[6] = picks[5]
    _rejected(keys, eligible, picks, u24, w, "picked twice")
