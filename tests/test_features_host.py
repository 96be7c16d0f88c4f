"""CPU: the review reader (bbgr.features.review_columns_from_jsonl) against
hand-written columns, and the host restatement (tests/features_ref.py) against
hand-computed labels and features, on a dump of twelve lines."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from features_ref import TAU_MS as TAU, features_ref  # noqa: E402

LINES = [
    dict(user_id="A", parent_asin="X", rating=5.0, helpful_vote=10, verified_purchase=True,
         timestamp=1000, title="Great", text="It's great great"),
    dict(user_id="B", parent_asin="X", rating=4.0, helpful_vote=0, verified_purchase=False,
         timestamp=TAU - 1, text="ok"),                                       # no title
    dict(user_id="A", parent_asin="Y", rating=2.5, helpful_vote=6, timestamp=2000, title="bad"),
    dict(user_id="A", parent_asin="Y", helpful_vote=99, timestamp=7, text="no rating"),
    dict(user_id="C", parent_asin="Z", rating=1, helpful_vote=5, title="", text=""),
    dict(parent_asin="Z", rating=3, helpful_vote=50, timestamp=9, text="no user"),
    dict(user_id="B", parent_asin="Y", rating=3.5, helpful_vote=7, verified_purchase=True,
         timestamp=TAU, text="don't don't DON'T stop"),
    dict(user_id="A", parent_asin="Z", rating=3.0, helpful_vote=6, timestamp=3 * TAU + 5,
         title="x", text="a b c"),
    dict(user_id="B", parent_asin="X", rating=5, helpful_vote=6, timestamp=TAU + 1, text="fine"),
    dict(user_id="A", parent_asin="X", rating=4.5, verified_purchase=True, timestamp=-1,
         text="rock'n'roll 42"),                                              # no helpful_vote
    dict(user_id="C", asin="X", rating=4, helpful_vote=8, timestamp=11, text="no parent_asin"),
    dict(user_id="C", parent_asin="X", rating=2, helpful_vote=0, timestamp=5, title=None,
         text="meh meh"),
]


@pytest.fixture(scope="module")
def read(tmp_path_factory):
    from bbgr.features import review_columns_from_jsonl
    p = tmp_path_factory.mktemp("reviews") / "reviews.jsonl"
    p.write_text("".join(json.dumps(r) + "\n" for r in LINES))
    return review_columns_from_jsonl(p)


def test_reader_columns_and_maps(read):
    cols, user2idx, item2idx = read
    assert user2idx == {"A": 0, "B": 1, "C": 2} and list(user2idx) == ["A", "B", "C"]
    assert item2idx == {"X": 0, "Y": 1, "Z": 2}
    want = dict(
        user=[0, 1, 0, 2, 1, 0, 1, 0, 2], item=[0, 0, 1, 2, 1, 2, 0, 0, 0],
        rating=[5, 4, 2.5, 1, 3.5, 3, 5, 4.5, 2], helpful_vote=[10, 0, 6, 5, 7, 6, 6, 0, 0],
        verified=[1, 0, 0, 0, 1, 0, 0, 1, 0],
        timestamp=[1000, TAU - 1, 2000, 0, TAU, 3 * TAU + 5, TAU + 1, -1, 5],
        ts_valid=[1, 1, 1, 0, 1, 1, 1, 1, 1],
        # "great it's great great", " ok", "bad ", " ", "don't" x 3 + "stop", "x a b c",
        # " fine", "rock'n" + "roll" (one inner apostrophe part, digits dropped), "meh meh"
        n_tokens=[4, 1, 1, 0, 4, 4, 1, 2, 2], n_unique_tokens=[2, 1, 1, 0, 2, 4, 1, 2, 1])
    dtypes = dict(user=np.int32, item=np.int32, rating=np.float32, helpful_vote=np.int32,
                  verified=np.uint8, timestamp=np.int64, ts_valid=np.bool_, n_tokens=np.int32,
                  n_unique_tokens=np.int32)
    assert len(cols) == 9
    for name, vals in want.items():
        got = getattr(cols, name)
        assert got.dtype == dtypes[name], name
        np.testing.assert_array_equal(got, np.asarray(vals, dtypes[name]), err_msg=name)


def test_reader_other_item_key(tmp_path):
    from bbgr.features import review_columns_from_jsonl
    p = tmp_path / "r.jsonl"
    p.write_text("".join(json.dumps(r) + "\n" for r in LINES))
    cols, user2idx, item2idx = review_columns_from_jsonl(p, item_id_key="asin")
    assert len(cols) == 1 and user2idx == {"C": 0} and item2idx == {"X": 0}


def test_tokenize():
    from bbgr.features import tokenize
    assert tokenize("It's GREAT, isn't it? 'quoted' o'neil's") == \
        ["it's", "great", "isn't", "it", "quoted", "o'neil", "s"]
    assert tokenize("") == [] and tokenize(None) == [] and tokenize("123 !!") == []


def test_restatement_hand_computed(read):
    cols, _, _ = read
    r = features_ref(cols, 3, 3)
    x = r["user_x64"]
    np.testing.assert_array_equal(r["total_reviews"], [4, 3, 2])
    np.testing.assert_array_equal(r["helpful_reviews"], [3, 2, 0])      # votes 5 and 0: not helpful
    # Ru 3/4, 2/3, 0 -> genuine, unlabeled, fake
    assert x[0, 0] == 0.75 and x[1, 0] == 2 / 3 and x[2, 0] == 0.0
    np.testing.assert_array_equal(r["user_y"], [1, -1, 0])
    # A: 5, 2.5 -> 2, 3, 4.5 -> 4: four bins once; B: 4, 3.5 -> 4, 5; C: 1, 2
    assert x[0, 1] == pytest.approx(math.log(4), rel=1e-15)
    assert x[1, 1] == pytest.approx(-(2 / 3) * math.log(2 / 3) - (1 / 3) * math.log(1 / 3),
                                    rel=1e-15)
    assert x[2, 1] == pytest.approx(math.log(2), rel=1e-15)
    np.testing.assert_array_equal(x[:, 2], [0.25, 1 / 3, 0.5])           # extremity
    # item means of ri: X (5,4,5,4,2) = 4, Y (2,4) = 3, Z (1,3) = 2
    np.testing.assert_array_equal(x[:, 3], [(1 + 1 + 1 + 0) / 4, (0 + 1 + 1) / 3, (1 + 2) / 2])
    # buckets A: 0, 0, 3, -1; B: 0 (TAU - 1), 1 (TAU), 1; C: 0 (one record has no timestamp)
    np.testing.assert_array_equal(x[:, 4], [1, 1, 0])
    assert x[2, 5] == 0.25                                               # (skip L = 0, 1/2) / 2
    assert x[0, 5] == (2 / 4 + 1 + 1 + 1) / 4
    g = 19 / 9
    assert r["stats"] == {"E": 9, "ts_min": -1, "ts_max": 3 * TAU + 5, "global_avg_len": g}
    assert x[2, 6] == (abs(0 - g) + abs(2 - g)) / 2
    assert r["user_x"].dtype == np.float32 and r["user_x"][1, 0] == np.float32(2 / 3)
    # item_x: the RAW rating's mean; X = 20.5 / 5
    np.testing.assert_array_equal(r["item_x"], np.asarray([[4.1, 5], [3, 2], [2, 2]], np.float32))
    ea = r["edge_attr"]
    m = float(np.float32(4.1))
    assert ea[0, 1] == np.float32(1 - (5 - m) / 4) and ea[0, 1] == pytest.approx(0.775, abs=1e-6)
    assert ea[2, 1] == np.float32(0.875) and ea[4, 1] == np.float32(0.875)   # 2.5, 3.5 vs 3
    np.testing.assert_array_equal(ea[:, 0], [1, 0, 0, 0, 1, 0, 0, 1, 0])
    np.testing.assert_array_equal(ea[:, 2], cols.rating)
    np.testing.assert_array_equal(ea[:, 4], [10, 0, 6, 5, 7, 6, 6, 0, 0])
    span = 3 * TAU + 6
    assert math.isnan(ea[3, 3]) and ea[7, 3] == 0.0 and ea[5, 3] == 1.0
    assert ea[0, 3] == np.float32(1001 / span)


def test_restatement_empty_rows_and_equal_timestamps(read):
    cols, _, _ = read
    r = features_ref(cols, 5, 4)
    assert np.isnan(r["user_x"][3:]).all() and (r["user_y"][3:] == -1).all()
    np.testing.assert_array_equal(r["item_x"][3], [0, 0])
    cols2 = type(cols)(**{**cols.__dict__, "timestamp": np.full(9, 77, np.int64), "ts_valid": None})
    r2 = features_ref(cols2, 3, 3)
    assert np.isnan(r2["edge_attr"][:, 3]).all()
    np.testing.assert_array_equal(r2["user_x64"][:, 4], [3, 2, 1])       # one bucket each
