"""GPU: the v2 feature passes (csrc/features_v2.hip) at the edges of the row
pass they share with csrc/features.hip (csrc/features.h), which the corpus of
tests/test_gpu_features_v2.py does not reach: user rows around the gap pass's
limit GAP_SHORT_ROW = 64, around the workgroup's stride 256 and around
FEAT_LONG_ROW = 512, item rows around 512, a long gap row with fewer than
three dated records, a long row with none, and more long gap rows than
FEAT_LONG_GRID = 256 workgroups, so that the long-row list needs a second trip.

The reference is tests/features_v2_ref.py and the comparison the one of
tests/test_gpu_features_v2.py: the exact columns exactly, the entropy, the
deviation, the discrepancy and ETG within 1 float32 ulp."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import features_ref as FR  # noqa: E402
import features_v2_ref as V  # noqa: E402
from test_gpu_features_v2 import _build, _columns, _compare, _np  # noqa: E402

GAP_SHORT_ROW = 64               # longer rows of bbgr_feat_gaps take one workgroup each
LONG_ROW = 512                   # FEAT_LONG_ROW: the same for the other row passes
LONG_GRID = 256                  # FEAT_LONG_GRID: workgroups striding over a long-row list
RATINGS = np.asarray([0.3, 1.1, 2.5, 2.9, 3.7, 4.3, 4.5, 5.0], np.float32)
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 66, 255, 256, 257, 511, 512, 513, 769]   # users 0.., all dated
U_FEW_TS = len(LENGTHS)          # 65 records, 2 of them dated: a long gap row with m < 3
U_NO_TS = U_FEW_TS + 1           # 513 records, none dated
U_MANY = U_NO_TS + 1             # 257 users of 65 records each
N_MANY = LONG_GRID + 1
N_USERS = U_MANY + N_MANY + 1    # the last user and the last item have no record
ITEM_LENGTHS = [511, 512, 513, 769]                                         # items 0..3
I_FILL, N_FILL = len(ITEM_LENGTHS), 50
N_ITEMS = I_FILL + N_FILL + 1
OUTPUT_KEYS = ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
               "helpful_reviews", "user_extra")


def _edge_columns():
    rng = np.random.default_rng(950)
    counts = np.asarray(LENGTHS + [65, 513] + [65] * N_MANY)
    user = np.repeat(np.arange(counts.size), counts)
    E = user.size
    item = rng.integers(I_FILL, I_FILL + N_FILL, E)
    picked = rng.permutation(E)[:sum(ITEM_LENGTHS)]
    item[picked] = np.repeat(np.arange(len(ITEM_LENGTHS)), ITEM_LENGTHS)
    ts = 1_200_000_000_000 + rng.integers(0, 3000 * FR.TAU_MS, E)
    ts_valid = rng.uniform(size=E) >= 0.1
    ts_valid[user < len(LENGTHS)] = True
    few = np.flatnonzero(user == U_FEW_TS)
    ts_valid[few] = False
    ts_valid[few[[7, 40]]] = True
    ts_valid[user == U_NO_TS] = False
    vocab = V._vocabulary()
    records = []
    for e in range(E):                        # a few words of the user's own window
        lo = int(user[e]) * 37 % (len(vocab) - 40)
        words = [vocab[k] for k in rng.integers(lo, lo + 40, int(rng.integers(0, 6))).tolist()]
        records.append(" ".join(w.upper() if j % 3 == 2 else w for j, w in enumerate(words)))
    order = rng.permutation(E)                # file order mixes all of it
    data, offsets = V.text_of([records[e] for e in order.tolist()])
    return types.SimpleNamespace(
        user=user[order].astype(np.int32), item=item[order].astype(np.int32),
        rating=rng.choice(RATINGS, E).astype(np.float32),
        helpful_vote=rng.choice(np.asarray([0, 0, 0, 1, 5, 6, 7, 20]), E).astype(np.int32),
        verified=(rng.uniform(size=E) < 0.5).astype(np.uint8),
        timestamp=ts[order].astype(np.int64), ts_valid=ts_valid[order],
        text=types.SimpleNamespace(data=data, offsets=offsets))


@pytest.fixture(scope="module")
def case():
    ns = _edge_columns()
    cols = _columns(ns)
    return (ns, cols, V.features_v2_ref(ns, N_USERS, N_ITEMS),
            _build(cols, N_USERS, N_ITEMS, feature_set="v2"))


def test_rows_are_what_the_docstring_lists(case):
    ns, _, ref, _ = case
    deg_u = np.bincount(ns.user, minlength=N_USERS)
    deg_i = np.bincount(ns.item, minlength=N_ITEMS)
    dated = np.bincount(ns.user, weights=ns.ts_valid, minlength=N_USERS).astype(np.int64)
    np.testing.assert_array_equal(deg_u[:len(LENGTHS)], LENGTHS)
    np.testing.assert_array_equal(dated[:len(LENGTHS)], LENGTHS)
    assert {GAP_SHORT_ROW + k for k in (-1, 0, 1)} <= set(LENGTHS)
    assert {LONG_ROW + k for k in (-1, 0, 1)} <= set(LENGTHS) and max(LENGTHS) > 3 * 256
    assert deg_u[U_FEW_TS] == GAP_SHORT_ROW + 1 and dated[U_FEW_TS] == 2
    assert deg_u[U_NO_TS] == LONG_ROW + 1 and dated[U_NO_TS] == 0
    assert (deg_u[U_MANY:U_MANY + N_MANY] == GAP_SHORT_ROW + 1).all()
    assert (dated[U_MANY:U_MANY + N_MANY] >= 3).all()
    # more long gap rows than workgroups: the long kernel's loop makes a second trip
    assert (deg_u > GAP_SHORT_ROW).sum() > LONG_GRID
    np.testing.assert_array_equal(deg_i[:I_FILL], ITEM_LENGTHS)
    assert deg_i[I_FILL:].max() <= LONG_ROW
    assert deg_u[-1] == 0 and deg_i[-1] == 0
    assert 20_000 < ns.user.size < 25_000
    assert ref["pooled_tokens"].sum() > 2 * ns.user.size > ref["pooled_unique"].sum()
    assert ref["pooled_unique"][len(LENGTHS) - 1] <= 40 < ref["pooled_tokens"][len(LENGTHS) - 1]
    assert set(np.unique(ns.rating).tolist()) == set(RATINGS.tolist())


def test_v2_edges_against_the_restatement(case):
    """Largest distances on MI355X: printed by the run (-s); above 1 is a bug."""
    _, _, ref, out = case
    _compare(out, ref, N_USERS, N_ITEMS)
    ux, ex = _np(out.user_x), _np(out.user_extra)
    for u in (0, N_USERS - 1):                # no record: the NaN row, unlabeled
        assert np.isnan(ux[u]).all() and np.isnan(ex[u]).all() and int(out.user_y[u]) == -1
    etg = ex[:, 1]
    assert (etg[[1, 2, U_FEW_TS, U_NO_TS]] == 0).all()        # fewer than three dated records
    assert (etg[4:len(LENGTHS)] > 0).all() and (etg[U_MANY:U_MANY + N_MANY] > 0).all()
    assert ux[U_NO_TS, 4] == 0
    np.testing.assert_array_equal(_np(out.item_x[-1]), [0, 0])


def test_two_builds_give_the_same_bits(case):
    _, cols, _, out = case
    again = _build(cols, N_USERS, N_ITEMS, feature_set="v2")
    for key in OUTPUT_KEYS:
        a, b = _np(getattr(out, key)), _np(getattr(again, key))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert out.stats == again.stats
