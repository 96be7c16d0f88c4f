"""GPU: build_credibility_graph(.., feature_set="v2") and
bbgr.text.pooled_token_counts (csrc/features_v2.hip) against the host
restatement tests/features_v2_ref.py (main_v2_.py:291-524) on the corpus
tests/test_features_v2_host.py checks on the host."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import features_v2_ref as V  # noqa: E402
import text_ref as TR  # noqa: E402

DEV = "cuda"
U, I = V.U, V.I
EXACT_USER_COLS = [0, 2, 4, 5]   # Ru, extremity ratio, burst count / n, pooled diversity
ULP_USER_COLS = [1, 3, 6]        # entropy, rating deviation, log-length discrepancy


def _columns(ns, **kw):
    from bbgr.features import ReviewColumns
    from bbgr.text import ReviewText
    c = dict(user=ns.user, item=ns.item, rating=ns.rating, helpful_vote=ns.helpful_vote,
             verified=ns.verified, timestamp=ns.timestamp, ts_valid=ns.ts_valid,
             text=ReviewText(ns.text.data, ns.text.offsets))
    c.update(kw)
    return ReviewColumns(**c)


def _build(cols, n_users=U, n_items=I, **kw):
    from bbgr.features import build_credibility_graph
    return build_credibility_graph(cols, n_users, n_items, device=DEV, **kw)


@pytest.fixture(scope="module")
def case():
    ns = V.corpus_columns(V.gpu_corpus())
    toks = V.record_tokens(ns.text)
    cols = _columns(ns)
    return ns, cols, V.features_v2_ref(ns, U, I, toks), _build(cols, feature_set="v2")


def _np(t):
    return t.cpu().numpy()


def _ulps(got, want):
    """Distance in float32 steps (non-negative values; a zero of either sign
    is zero: numpy yields -0.0 for the entropy of one bin); the NaNs must
    coincide."""
    got, want = got + np.float32(0), want + np.float32(0)      # -0.0 + 0.0 = +0.0
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    d[nan] = 0
    return d


def _compare(out, ref, n_users, n_items):
    """Exact: everything but user columns 1, 3, 6 and ETG; those within 1
    float32 ulp (double sums in another order and the device log / log1p move
    a double by about n * 2^-53; all terms are of one sign, so a float32
    result can differ only where the double straddles a rounding boundary).
    Prints the largest distance per column."""
    from bbgr.features import CredibilityGraphV2
    E = ref["stats"]["E"]
    assert isinstance(out, CredibilityGraphV2)
    assert out.user_x.shape == (n_users, 7) and out.user_extra.shape == (n_users, 2)
    assert out.user_extra.dtype == torch.float32 and out.user_extra.is_cuda
    assert out.edge_attr.shape == (E, 5) and out.item_x.shape == (n_items, 2)
    for key in ("src", "dst", "user_y", "total_reviews", "helpful_reviews"):
        np.testing.assert_array_equal(_np(getattr(out, key)), ref[key], err_msg=key)
    want = dict(ref["stats"])
    got = dict(out.stats)
    assert got.pop("global_avg_lenlog") == pytest.approx(want.pop("global_avg_lenlog"),
                                                         rel=1e-13, abs=0)
    assert got == want
    np.testing.assert_array_equal(_np(out.item_x), ref["item_x"])
    np.testing.assert_array_equal(_np(out.edge_attr), ref["edge_attr"])
    ux, rx = _np(out.user_x), ref["user_x"]
    ex, rex = _np(out.user_extra), ref["user_extra"]
    np.testing.assert_array_equal(ux[:, EXACT_USER_COLS], rx[:, EXACT_USER_COLS])
    np.testing.assert_array_equal(ex[:, 0], rex[:, 0])
    d = _ulps(np.ascontiguousarray(np.c_[ux[:, ULP_USER_COLS], ex[:, 1]]),
              np.ascontiguousarray(np.c_[rx[:, ULP_USER_COLS], rex[:, 1]]))
    print("largest ulp distance per column (entropy, deviation, discrepancy, ETG):",
          d.max(axis=0) if d.size else d)
    assert d.size == 0 or d.max() <= 1


def test_v2_against_the_restatement(case):
    """Largest distances on MI355X: printed by the run (-s); above 1 is a bug."""
    ns, _, ref, out = case
    _compare(out, ref, U, I)
    assert np.isnan(_np(out.user_x[U - 1])).all() and np.isnan(_np(out.user_extra[U - 1])).all()
    assert int(out.user_y[U - 1]) == -1
    etg = _np(out.user_extra[:, 1])
    for u, k in V.TS_COUNT_USERS.items():
        if k < 3:
            assert etg[u] == 0
    assert etg[V.REPEAT_USER] == 0 and etg[0] > 5        # one bin; all 366 bins


def test_pooled_token_counts(case):
    from bbgr.text import ReviewText, pooled_token_counts
    ns, _, ref, _ = case
    text = ReviewText(ns.text.data, ns.text.offsets)
    tok, uniq, info = pooled_token_counts(text, ns.user, U, DEV)
    assert tok.dtype == torch.int64 and uniq.dtype == torch.int32 and tok.is_cuda
    np.testing.assert_array_equal(_np(tok), ref["pooled_tokens"])
    np.testing.assert_array_equal(_np(uniq), ref["pooled_unique"])
    assert info["rechecked"] == len(V.KELVIN_RECORDS)
    assert info["kelvin_records"] == sum(V.KELVIN_RECORDS.values())
    assert info["tokens"] == int(ref["pooled_tokens"].sum())
    # a hash of 8 bits: collisions everywhere, counts still exact, more groups handed back
    tok8, uniq8, info8 = pooled_token_counts(text, ns.user, U, DEV, _hash_mask=0xFF)
    assert torch.equal(tok8, tok) and torch.equal(uniq8, uniq)
    assert info8["rechecked"] > info["rechecked"]
    # groups on the device; outputs as leading views of sentinel-filled buffers
    big_t = torch.full((U + 64,), -7, dtype=torch.int64, device=DEV)
    big_u = torch.full((U + 64,), -7, dtype=torch.int32, device=DEV)
    tok_v, uniq_v, _ = pooled_token_counts(text, torch.as_tensor(ns.user).to(DEV), U, DEV,
                                           out=(big_t[:U], big_u[:U]))
    assert torch.equal(tok_v, tok) and torch.equal(uniq_v, uniq)
    assert tok_v.data_ptr() == big_t.data_ptr()
    assert bool((big_t[U:] == -7).all()) and bool((big_u[U:] == -7).all())
    with pytest.raises(ValueError, match="group id out of range"):
        pooled_token_counts(text, np.where(ns.user == 3, U, ns.user), U, DEV)


def test_main_is_untouched_by_the_argument(case):
    _, cols, _, _ = case
    a, b = _build(cols), _build(cols, feature_set="main")
    from bbgr.features import CredibilityGraph
    assert type(a) is CredibilityGraph and type(b) is CredibilityGraph
    for key in ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
                "helpful_reviews"):
        x, y = _np(getattr(a, key)), _np(getattr(b, key))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key
    assert a.stats == b.stats and "global_avg_lenlog" not in a.stats


def test_two_v2_builds_are_bitwise_identical(case):
    _, cols, _, out = case
    again = _build(cols, feature_set="v2")
    for key in ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
                "helpful_reviews", "user_extra"):
        a, b = _np(getattr(out, key)), _np(getattr(again, key))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert out.stats == again.stats


def _small(E, seed, n_users=9, n_items=5, dated=True):
    import types
    rng = np.random.default_rng(seed)
    records = TR.random_records(E, seed, max_tokens=12)
    data, offsets = V.text_of(records)
    return types.SimpleNamespace(
        user=rng.integers(0, n_users, E).astype(np.int32),
        item=rng.integers(0, n_items, E).astype(np.int32),
        rating=rng.choice(np.array([1, 2.5, 3, 4.5, 5]), E).astype(np.float32),
        helpful_vote=rng.integers(0, 12, E).astype(np.int32),
        verified=rng.integers(0, 2, E).astype(np.uint8),
        timestamp=(1_200_000_000_000 + rng.integers(0, 900 * 86_400_000, E)).astype(np.int64),
        ts_valid=np.full(E, dated), text=types.SimpleNamespace(data=data, offsets=offsets))


@pytest.mark.parametrize("which", ["no_records", "no_timestamps", "dated"])
def test_small_cases(which):
    ns = _small(0 if which == "no_records" else 70, 5, dated=which == "dated")
    ref = V.features_v2_ref(ns, 9, 5)
    out = _build(_columns(ns), 9, 5, feature_set="v2")
    _compare(out, ref, 9, 5)
    has = _np(out.total_reviews) > 0
    if which == "no_records":
        assert not has.any() and np.isnan(_np(out.user_extra)).all()
        assert out.stats["global_avg_lenlog"] == 0.0
    if which == "no_timestamps":
        assert (_np(out.user_extra[:, 1])[has] == 0).all() and (_np(out.user_x[:, 4])[has] == 0).all()


def test_tokens_from_the_columns_when_given(case):
    """n_tokens is taken from the columns when they hold it: the same bits."""
    ns, _, _, out = case
    n_tok = np.asarray([len(t) for t in V.record_tokens(ns.text)], np.int32)
    again = _build(_columns(ns, n_tokens=n_tok), feature_set="v2")
    assert torch.equal(again.user_x.view(torch.int32), out.user_x.view(torch.int32))
    assert torch.equal(again.user_extra.view(torch.int32), out.user_extra.view(torch.int32))


def test_jsonl_to_v2_to_the_slas_graph(tmp_path):
    from bbgr.cred_train import SlasGraph
    from bbgr.features import review_columns_from_jsonl
    rng = np.random.default_rng(3)
    records = TR.random_records(120, 21, max_tokens=15)
    path = tmp_path / "reviews.jsonl"
    with open(path, "w", encoding="utf-8") as f:
        for k, s in enumerate(records):
            f.write(json.dumps({
                "user_id": f"u{int(rng.integers(0, 20))}", "parent_asin": f"i{int(rng.integers(0, 15))}",
                "rating": float(rng.integers(1, 6)), "helpful_vote": int(rng.integers(0, 12)),
                "verified_purchase": bool(k % 2), "title": s[:10], "text": s,
                "timestamp": 1_600_000_000_000 + int(rng.integers(0, 10**10))}) + "\n")
    cols, user2idx, item2idx = review_columns_from_jsonl(path, tokens="device", device=DEV)
    assert cols.text is not None
    out = _build(cols, len(user2idx), len(item2idx), feature_set="v2")
    assert torch.isfinite(out.user_x).all() and torch.isfinite(out.user_extra).all()
    g = SlasGraph((out.src, out.dst), out.edge_attr, out.user_x, out.user_y, out.item_x, DEV)
    assert g is not None
