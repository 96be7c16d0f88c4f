"""GPU: bbgr.features.build_credibility_graph (csrc/features.hip) against the
host restatement tests/features_ref.py (main.py:153-196, :247-373, :423-570)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import features_ref as FR  # noqa: E402

DEV = "cuda"
TAU = FR.TAU_MS
U, I = 300, 200
HUB = 5500                     # records of the hub user (0) and of the hub item (0): long rows
EXACT_USER_COLS = [0, 2, 4]    # Ru, extremity_ratio, review_burst_count
ULP_USER_COLS = [1, 3, 5, 6]   # entropy, rating deviation, lexical diversity, length discrepancy
# (records, helpful) of users 1..6: Ru exactly 3/10 and 7/10, and one each side of both
THRESHOLD_USERS = {1: (10, 3), 2: (10, 7), 3: (100, 29), 4: (100, 31), 5: (100, 69), 6: (100, 71)}


def _cols(**kw):
    from bbgr.features import ReviewColumns
    return ReviewColumns(**kw)


def _main_columns():
    rng = np.random.default_rng(2024)
    n_base = 8600
    user = [rng.integers(7, U - 1, n_base)]                 # user U - 1 has no record
    item = [rng.integers(1, I - 1, n_base)]                 # item I - 1 has no record
    user.append(np.zeros(HUB, np.int64))                    # the hub user: every pair repeats
    item.append(rng.integers(0, I - 1, HUB))
    user.append(rng.integers(7, U - 1, HUB))                # the hub item
    item.append(np.zeros(HUB, np.int64))
    for u, (n, _) in THRESHOLD_USERS.items():
        user.append(np.full(n, u))
        item.append(rng.integers(1, I - 1, n))
    user, item = np.concatenate(user), np.concatenate(item)
    E = user.size
    # multiples of 0.5 (double sums are exact in any order): the half-even ties 0.5, 2.5, 3.5,
    # 4.5, and 0, 5.5, 7 for the clamp
    rating = rng.choice(np.array([0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 7]), E)
    helpful = rng.choice(np.array([0, 0, 0, 1, 5, 6, 7, 20]), E)
    for u, (n, h) in THRESHOLD_USERS.items():
        helpful[user == u] = np.concatenate([np.full(h, 6), np.full(n - h, 5)])
    n_tokens = rng.integers(0, 60, E)
    n_tokens[rng.uniform(size=E) < 0.1] = 0                 # L = 0
    n_unique = np.where(n_tokens > 0, rng.integers(0, 60, E) % np.maximum(n_tokens, 1) + 1, 0)
    ts = rng.integers(-5 * TAU, 400 * TAU, E)               # 405 buckets: they repeat, some < 0
    edge = np.flatnonzero(user == 10)                       # pairs at k TAU - 1 and k TAU
    for j, k in enumerate([-2, 0, 3]):
        ts[edge[2 * j]], ts[edge[2 * j + 1]] = k * TAU - 1, k * TAU
    ts_valid = rng.uniform(size=E) >= 0.1
    ts_valid[edge[:6]] = True
    verified = rng.uniform(size=E) < 0.5
    order = rng.permutation(E)                              # file order mixes all of it
    return _cols(user=user[order].astype(np.int32), item=item[order].astype(np.int32),
                 rating=rating[order].astype(np.float32),
                 helpful_vote=helpful[order].astype(np.int32),
                 verified=verified[order].astype(np.uint8), timestamp=ts[order].astype(np.int64),
                 n_tokens=n_tokens[order].astype(np.int32),
                 n_unique_tokens=n_unique[order].astype(np.int32), ts_valid=ts_valid[order])


def _build(cols, n_users=U, n_items=I):
    from bbgr.features import build_credibility_graph
    return build_credibility_graph(cols, n_users, n_items, device=DEV)


@pytest.fixture(scope="module")
def main_case():
    cols = _main_columns()
    return cols, FR.features_ref(cols, U, I), _build(cols)


def _np(t):
    return t.cpu().numpy()


def _ulps(got, want):
    """Distance in float32 steps (non-negative values); the NaNs must coincide."""
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    d[nan] = 0
    return d


def _compare(out, ref, n_users, n_items):
    """Everything exact but the four order- and log-dependent user features,
    those within 1 float32 ulp (their double sums depend on order and on the
    device log, about n * 2^-53 relative: a float32 result can differ only
    where the double straddles a rounding boundary). Prints the largest
    distance seen."""
    E = ref["stats"]["E"]
    assert out.src.dtype == torch.int32 and out.dst.dtype == torch.int32
    assert out.user_y.dtype == torch.int64 and out.total_reviews.dtype == torch.int32
    assert out.edge_attr.shape == (E, 5) and out.user_x.shape == (n_users, 7)
    assert out.item_x.shape == (n_items, 2) and out.user_y.shape == (n_users,)
    for t in (out.src, out.dst, out.edge_attr, out.user_x, out.user_y, out.item_x):
        assert t.is_cuda
    for key in ("src", "dst", "user_y", "total_reviews", "helpful_reviews"):
        np.testing.assert_array_equal(_np(getattr(out, key)), ref[key], err_msg=key)
    assert out.stats == ref["stats"]
    np.testing.assert_array_equal(_np(out.item_x), ref["item_x"])
    np.testing.assert_array_equal(_np(out.edge_attr), ref["edge_attr"])      # NaN == NaN here
    ux, rx = _np(out.user_x), ref["user_x"]
    np.testing.assert_array_equal(ux[:, EXACT_USER_COLS], rx[:, EXACT_USER_COLS])
    d = _ulps(np.ascontiguousarray(ux[:, ULP_USER_COLS]),
              np.ascontiguousarray(rx[:, ULP_USER_COLS]))
    print("largest ulp distance per column (entropy, deviation, diversity, discrepancy):",
          d.max(axis=0) if d.size else d)
    assert d.size == 0 or d.max() <= 1


def test_main_case_is_what_the_issue_lists(main_case):
    cols, ref, _ = main_case
    E = len(cols)
    assert 19_000 < E < 21_000
    deg_u, deg_i = np.bincount(cols.user, minlength=U), np.bincount(cols.item, minlength=I)
    assert deg_u[0] > 5000 and deg_i[0] > 5000 and deg_u[U - 1] == 0 and deg_i[I - 1] == 0
    for r in (0, 0.5, 2.5, 3.5, 4.5, 5.5, 7):
        assert (cols.rating == r).any()
    assert (cols.helpful_vote == 5).any() and (cols.helpful_vote == 6).any()
    assert (cols.n_tokens == 0).any() and (~cols.ts_valid).any()
    assert (cols.timestamp[cols.ts_valid] < 0).any()
    t10 = set(cols.timestamp[cols.user == 10].tolist())
    assert all({k * TAU - 1, k * TAU} <= t10 for k in (-2, 0, 3))
    pairs = cols.user.astype(np.int64) * I + cols.item
    assert np.unique(pairs).size < E                         # duplicate (user, item) records
    assert ref["user_x64"][0, 4] > 100                       # repeated buckets
    # users 1..6: exactly 0.3 -> fake, exactly 0.7 -> genuine, and either side of both
    np.testing.assert_array_equal(ref["user_x64"][1:7, 0], [0.3, 0.7, 0.29, 0.31, 0.69, 0.71])
    np.testing.assert_array_equal(ref["user_y"][1:7], [0, 1, 0, -1, -1, 1])


def test_main_case(main_case):
    """Largest distance observed on MI355X: 0 ulp in all four columns (a
    difference needs a double within ~1e-16 relative of a float32 rounding
    boundary); above 1 is a bug."""
    _, ref, out = main_case
    _compare(out, ref, U, I)
    ux = _np(out.user_x)
    assert np.isnan(ux[U - 1]).all() and int(out.user_y[U - 1]) == -1
    np.testing.assert_array_equal(_np(out.item_x[I - 1]), [0, 0])
    ea = _np(out.edge_attr)
    np.testing.assert_array_equal(np.isnan(ea[:, 3]), ~np.asarray(main_case[0].ts_valid, bool))
    assert not np.isnan(ea[:, [0, 1, 2, 4]]).any()


def test_two_builds_are_bitwise_identical(main_case):
    cols, _, out = main_case
    again = _build(cols)
    for key in ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
                "helpful_reviews"):
        a, b = _np(getattr(out, key)), _np(getattr(again, key))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert out.stats == again.stats


def test_device_tensors_as_columns(main_case):
    cols, _, out = main_case
    on_dev = _cols(**{k: torch.as_tensor(np.asarray(v)).to(DEV)
                      for k, v in cols.__dict__.items()})
    again = _build(on_dev)
    assert torch.equal(again.user_x.view(torch.int32), out.user_x.view(torch.int32))
    assert torch.equal(again.edge_attr.view(torch.int32), out.edge_attr.view(torch.int32))


def _small(seed, E, n_users=9, n_items=5, **kw):
    rng = np.random.default_rng(seed)
    c = dict(user=rng.integers(0, n_users, E).astype(np.int32),
             item=rng.integers(0, n_items, E).astype(np.int32),
             rating=rng.choice(np.array([1, 2.5, 3, 4.5, 5]), E).astype(np.float32),
             helpful_vote=rng.integers(0, 12, E).astype(np.int32),
             verified=rng.integers(0, 2, E).astype(np.uint8),
             timestamp=rng.integers(-3 * TAU, 3 * TAU, E).astype(np.int64),
             n_tokens=rng.integers(0, 9, E).astype(np.int32),
             n_unique_tokens=rng.integers(0, 9, E).astype(np.int32), ts_valid=None)
    c.update(kw)
    return _cols(**c)


@pytest.mark.parametrize("case", ["no_records", "one_record", "equal_timestamps", "no_timestamps",
                                  "ts_valid_none"])
def test_degenerate(case):
    if case == "no_records":
        cols = _small(0, 0)
    elif case == "one_record":
        cols = _small(1, 1, ts_valid=np.ones(1, bool))
    elif case == "equal_timestamps":
        cols = _small(2, 40, timestamp=np.full(40, 5 * TAU + 3, np.int64))
    elif case == "no_timestamps":
        cols = _small(3, 40, ts_valid=np.zeros(40, bool))
    else:
        cols = _small(4, 40)
    ref = FR.features_ref(cols, 9, 5)
    out = _build(cols, 9, 5)
    _compare(out, ref, 9, 5)
    ts_norm = _np(out.edge_attr[:, 3])
    if case == "ts_valid_none":
        assert not np.isnan(ts_norm).any() and ts_norm.min() == 0 and ts_norm.max() == 1
    else:
        assert np.isnan(ts_norm).all()
    if case == "no_records":
        assert out.stats == {"E": 0, "ts_min": None, "ts_max": None, "global_avg_len": 0.0}
        assert np.isnan(_np(out.user_x)).all() and (_np(out.user_y) == -1).all()
        assert not _np(out.item_x).any() and not _np(out.total_reviews).any()
    if case in ("no_timestamps", "no_records"):
        assert out.stats["ts_min"] is None and out.stats["ts_max"] is None
        assert (_np(out.user_x[:, 4])[_np(out.total_reviews) > 0] == 0).all()
    if case == "equal_timestamps":
        np.testing.assert_array_equal(_np(out.user_x[:, 4]),
                                      np.where(_np(out.total_reviews) > 0,
                                               _np(out.total_reviews) - 1, np.nan))


def _healthy():
    cols = _small(5, 30)
    _compare(_build(cols, 9, 5), FR.features_ref(cols, 9, 5), 9, 5)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["user", "item", "bucket_range", "span"])
def test_contract_errors_come_before_the_launch(case):
    from bbgr._lib import BbgrError
    if case == "user":
        user = np.asarray([0, 9, 3], np.int32)
        with pytest.raises(ValueError, match="user id out of range"):
            _build(_small(6, 3, user=user), 9, 5)
        with pytest.raises(ValueError, match="user id out of range"):
            _build(_small(6, 3, user=torch.as_tensor(user).to(DEV)), 9, 5)
    elif case == "item":
        with pytest.raises(ValueError, match="item id out of range"):
            _build(_small(6, 3, item=np.asarray([0, -1, 3], np.int32)), 9, 5)
    elif case == "bucket_range":
        ts = np.asarray([0, 2**31 * TAU, 7], np.int64)
        with pytest.raises(BbgrError, match="BBGR_ERR_INVALID.*timestamp"):
            _build(_small(6, 3, timestamp=ts), 9, 5)
    else:
        # buckets fit int32, but ts - ts_min is no longer an exact double everywhere
        ts = np.asarray([-5, 2**53 - 5, 7], np.int64)
        with pytest.raises(ValueError, match="timestamp.*2\\^53"):
            _build(_small(6, 3, timestamp=ts), 9, 5)
        out = _build(_small(6, 3, timestamp=ts - np.asarray([0, 1, 0])), 9, 5)   # 2^53 - 1: fine
        assert float(out.edge_attr[1, 3]) == 1.0 and float(out.edge_attr[0, 3]) == 0.0
    _healthy()


def test_feeds_the_slas_graph(main_case):
    """SlasGraph over the device outputs builds the subgraph that SlasGraph
    over the restatement's arrays builds: same picks, same bits."""
    from bbgr.cred_train import SlasGraph
    _, ref, out = main_case
    g = SlasGraph((out.src, out.dst), out.edge_attr, out.user_x, out.user_y, out.item_x, DEV)
    h = SlasGraph((ref["src"], ref["dst"]), ref["edge_attr"], ref["user_x"], ref["user_y"],
                  ref["item_x"], DEV)
    seeds = np.random.default_rng(8).permutation(U - 1)[:64].astype(np.int64)
    seeds[0] = 0                                             # the hub user
    got = g.build_subgraph(seeds, "early", counter=0)
    want = h.build_subgraph(seeds, "early", counter=0)
    assert set(got) == set(want) and got["bs"] == want["bs"] == 64
    assert got["e_u2i"].shape[1] > 64 and got["users_global"].numel() > 64
    for key in got:
        if key != "bs":
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
