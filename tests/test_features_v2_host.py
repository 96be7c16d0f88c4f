"""CPU: the host restatement tests/features_v2_ref.py on a hand-worked case,
and the properties of the GPU test's corpus that tests/test_gpu_features_v2.py
relies on."""
import math
import types

import numpy as np
import pytest

import features_ref as FR
import features_v2_ref as V
import text_ref as TR

DAY_MS, DAY_S = 86_400_000, 86_400


def _hand_case():
    a0 = 1_600_000_000_000                     # milliseconds
    b0 = 1_500_000_000                         # seconds
    c0 = 1_700_000_000_000 // DAY_MS * DAY_MS  # the start of a day bucket
    rows = [  # user, item, rating, timestamp, text          (file order)
        (0, 0, 5.0, a0, "a b"),
        (1, 0, 4.0, b0, "x x x"),
        (2, 0, 2.0, c0 + 5, "Good good movie"),
        (0, 1, 1.0, a0 + DAY_MS * 3 // 2, "c"),
        (1, 1, 4.0, b0 + 2 * DAY_S + 100, "x"),
        (0, 0, 2.5, a0 + DAY_MS * 3 // 2 + DAY_MS * 13 // 4, ""),
        (1, 1, 3.0, b0 + 4 * DAY_S + 200, "x y"),
        (2, 1, 5.0, c0 + 9, "GOOD film"),
    ]
    data, offsets = V.text_of([r[4] for r in rows])
    n = len(rows)
    return types.SimpleNamespace(
        user=np.asarray([r[0] for r in rows], np.int32),
        item=np.asarray([r[1] for r in rows], np.int32),
        rating=np.asarray([r[2] for r in rows], np.float32),
        helpful_vote=np.zeros(n, np.int32), verified=np.zeros(n, np.uint8),
        timestamp=np.asarray([r[3] for r in rows], np.int64), ts_valid=None,
        text=types.SimpleNamespace(data=data, offsets=offsets))


def test_hand_worked_case():
    """Three users, two items, eight records.

    Item means of the raw rating: item 0 has 5, 4, 2, 2.5 -> 13.5 / 4 = 3.375;
    item 1 has 1, 4, 3, 5 -> 13 / 4 = 3.25.
    Token counts L in file order: 2, 3, 3, 1, 1, 0, 2, 2; g = global_avg_lenlog
    = (3 ln 3 + 2 ln 4 + 2 ln 2 + 0) / 8 (log1p of 2, 3, 1, 0).

    User 0 (ratings 5, 1, 2.5; times in ms 1.5 and 3.25 days apart):
      column 3 = (|5 - 3.375| + |1 - 3.25| + |2.5 - 3.375|) / 3 = 4.75 / 3
      column 4 = 0 (three day buckets); column 5 = |{a, b, c}| / 3 = 1
      RNR = 2 / 3 (stars 5, 1, and round(2.5) = 2); the gaps fall in bins 1
      and 3: ETG = -2 (1/2) ln (1/2) = ln 2.
    User 1 (ratings 4, 4, 3; times in seconds, 2 days + 100 s apart twice):
      column 3 = (0.625 + 0.75 + 0.25) / 3; column 5 = |{x, y}| / 6 = 1 / 3
      column 4 = 2 / 3: the buckets are ts // 86 400 000 of the raw values,
      and three values in seconds a few days apart share one
      RNR = 0; both gaps in bin 2: ETG = 0.
    User 2 (ratings 2, 5; two times in one day bucket):
      column 3 = (1.375 + 1.75) / 2 = 1.5625; column 4 = 1 / 2
      column 5: "Good good movie" has 2 distinct, "GOOD film" 2, their sum 4,
      but pooled {good, movie, film} = 3 of 5 tokens = 0.6
      RNR = 1 / 2; two timestamps: ETG = 0.
    Column 6 = mean |log1p(L) - g| over the user's records."""
    ref = V.features_v2_ref(_hand_case(), 3, 2)
    x, extra = ref["user_x64"], ref["user_extra64"]
    g = (3 * math.log(3) + 2 * math.log(4) + 2 * math.log(2)) / 8
    assert ref["stats"]["global_avg_lenlog"] == pytest.approx(g, rel=1e-15)
    np.testing.assert_allclose(x[:, 3], [4.75 / 3, 1.625 / 3, 1.5625], rtol=1e-15)
    np.testing.assert_array_equal(x[:, 4], [0, 2 / 3, 0.5])
    np.testing.assert_array_equal(x[:, 5], [1.0, 2 / 6, 3 / 5])
    lens = {0: (2, 1, 0), 1: (3, 1, 2), 2: (3, 2)}
    want6 = [sum(abs(math.log1p(L) - g) for L in lens[u]) / len(lens[u]) for u in range(3)]
    np.testing.assert_allclose(x[:, 6], want6, rtol=1e-14)
    np.testing.assert_array_equal(extra[:, 0], [2 / 3, 0.0, 0.5])
    assert extra[0, 1] == pytest.approx(math.log(2), rel=1e-15)
    assert extra[1, 1] == 0 and extra[2, 1] == 0
    np.testing.assert_array_equal(ref["pooled_unique"], [3, 2, 3])
    np.testing.assert_array_equal(ref["pooled_tokens"], [3, 6, 5])
    # per-record distinct counts of user 2 add to more than its pooled count
    toks = V.record_tokens(_hand_case().text)
    assert len(set(toks[2])) + len(set(toks[7])) == 4 > ref["pooled_unique"][2]
    # columns 0 to 2, labels and the graph pass are main.py's
    main = FR.features_ref(types.SimpleNamespace(
        **{k: v for k, v in vars(_hand_case()).items() if k != "text"},
        n_tokens=np.asarray([len(t) for t in toks], np.int32),
        n_unique_tokens=np.asarray([len(set(t)) for t in toks], np.int32)), 3, 2)
    np.testing.assert_array_equal(x[:, :3], main["user_x64"][:, :3])
    np.testing.assert_array_equal(ref["edge_attr"], main["edge_attr"])


def test_ts_to_days_units():
    assert V.ts_to_days(10**12) == 10**12 / 1000.0 / 86400.0          # milliseconds from 10^12 on
    assert V.ts_to_days(10**12 - 1) == (10**12 - 1) / 86400.0         # seconds below
    assert V.ts_to_days(-5) == -5 / 86400.0


@pytest.fixture(scope="module")
def corpus():
    c = V.gpu_corpus()
    ns = V.corpus_columns(c)
    toks = V.record_tokens(ns.text)
    return c, ns, toks, V.features_v2_ref(ns, V.U, V.I, toks)


def test_corpus_is_what_the_issue_lists(corpus):
    c, ns, toks, ref = corpus
    E = len(c["records"])
    assert 19_000 < E < 21_000
    deg_u = np.bincount(c["user"], minlength=V.U)
    deg_i = np.bincount(c["item"], minlength=V.I)
    assert deg_u[0] == V.HUB and deg_i[0] > 5000 and deg_u[V.U - 1] == 0 and deg_i[V.I - 1] == 0
    for r in (0, 2.5, 5.5, 7):
        assert (c["rating"] == r).any()
    ts, ok = c["timestamp"], c["ts_valid"]
    assert (ts[ok] >= V.MS_FROM).any() and ((ts[ok] > 0) & (ts[ok] < V.MS_FROM)).any()
    assert (ts[ok] < 0).any() and 0.05 < (~ok).mean() < 0.15
    for u, k in V.TS_COUNT_USERS.items():
        assert len(ref["user_days"].get(u, [])) == k
    assert (V.gap_bins(ref["user_days"][V.REPEAT_USER]) == 0).all()
    pair_bins = V.gap_bins(ref["user_days"][V.EXACT_USER])[::2]
    assert all(b in (k, k - 1) for b, k in zip(pair_bins, V.EXACT_K))
    assert min(len(t) for t in toks) == 0 and max(len(t) for t in toks) > 50   # 0 - 60 words a record
    assert sum(TR.has_kelvin(TR.encode(s)) for s in c["records"]) == 3
    joined = " ".join(c["records"])
    assert "İ" in joined and "’" in joined and "é" in joined and "'" in joined
    assert any("'" in t for t in set().union(*map(set, toks)))
    # users reuse words across records in mixed case: pooled below the sum of per-record counts
    per_record = np.zeros(V.U, np.int64)
    np.add.at(per_record, c["user"], [len(set(t)) for t in toks])
    assert (ref["pooled_unique"][deg_u > 1] < per_record[deg_u > 1]).any()
    assert ref["pooled_unique"][0] < 200 < ref["pooled_tokens"][0]


def test_no_two_tokens_of_the_corpus_share_a_hash(corpus):
    """The condition under which the GPU test may demand that only the users
    with a U+212A record are handed back; with 8 bits they collide."""
    distinct = set().union(*map(set, corpus[2]))
    assert len(distinct) > 1900
    assert len({TR.token_hash(t.encode()) for t in distinct}) == len(distinct)
    assert len({TR.token_hash(t.encode(), 0xFF) for t in distinct}) <= 256


def test_corpus_checks_the_gpu_test_relies_on(corpus):
    c, _, _, ref = corpus
    has = np.bincount(c["user"], minlength=V.U) > 0
    assert ref["col6_sum"][has].min() >= 1e-3               # 1 ulp of column 6 means something
    hub_bins = V.gap_bins(ref["user_days"][0])
    assert np.unique(hub_bins).size == 366                   # every bin, the cap among them
    assert (hub_bins == 0).any() and (hub_bins == 365).sum() > 1
    # a gap whose floor is not the difference of the day buckets ts // TAU_MS
    differs = 0
    for u in range(V.U):
        rec = np.flatnonzero((c["user"] == u) & c["ts_valid"])
        if rec.size < 2:
            continue
        ts = c["timestamp"][rec].tolist()
        order = np.argsort([V.ts_to_days(t) for t in ts], kind="stable")
        days = [V.ts_to_days(ts[k]) for k in order]
        bucket = [ts[k] // FR.TAU_MS for k in order]
        differs += sum(math.floor(days[j + 1] - days[j]) != bucket[j + 1] - bucket[j]
                       for j in range(len(days) - 1))
    assert differs > 0
