"""Host restatement of what bbgr.features computes (the label, feature and
graph passes, main.py:153-196, :247-373, :423-570) over numeric review
columns: records are filed under their user and their item in file order, then
every quantity is a plain Python loop or sum over such a list, in Python float
(double), rounded to float32 only at the very end, where the reference's
``np.asarray(.., float32)`` rounds. Sums run in file order, the order in which
the reference's per-record loops add. The reference for
tests/test_features_host.py, tests/test_gpu_features.py and
tests/test_gpu_features_edges.py.
A helper, not a test module."""
import math

import numpy as np

TAU_MS = 86_400_000        # one day: the width of a burst bucket
HELPFUL_ABOVE = 5          # a review is helpful with more votes than this
GENUINE_FROM, FAKE_UPTO = 0.7, 0.3


def star(rating: float) -> int:
    """The rating as a whole star in 1..5; round() breaks ties to even."""
    return min(5, max(1, round(float(rating))))


def label_of(ru: float) -> int:
    if ru >= GENUINE_FROM:
        return 1
    return 0 if ru <= FAKE_UPTO else -1


def _filed(keys):
    """key -> the record ids that carry it, ascending (file order)."""
    out = {}
    for e, k in enumerate(keys):
        out.setdefault(k, []).append(e)
    return out


def user_sum_terms(cols) -> dict:
    """Per record, the double terms whose per-user sums features_ref divides
    into user columns 3, 5 and 6, formed exactly as features_ref forms them
    (a record without words adds nothing to column 5: its term is 0.0), as
    float64 arrays. For an order-free mean (math.fsum) over a user's records:
    tests/test_gpu_features_edges.py."""
    item = np.asarray(cols.item).tolist()
    rating = np.asarray(cols.rating, np.float32).astype(np.float64).tolist()
    words = np.asarray(cols.n_tokens).tolist()
    distinct = np.asarray(cols.n_unique_tokens).tolist()
    n_rec = len(item)
    stars = [star(r) for r in rating]
    mean_star = {i: sum(stars[e] for e in recs) / len(recs) for i, recs in _filed(item).items()}
    avg_words = sum(words) / max(n_rec, 1)
    return {
        3: np.asarray([abs(stars[e] - mean_star[item[e]]) for e in range(n_rec)], np.float64),
        5: np.asarray([distinct[e] / words[e] if words[e] > 0 else 0.0 for e in range(n_rec)],
                      np.float64),
        6: np.asarray([abs(words[e] - avg_words) for e in range(n_rec)], np.float64),
    }


def features_ref(cols, num_users: int, num_items: int) -> dict:
    """Every output of bbgr.features.build_credibility_graph as numpy arrays
    (plus ``user_x64``: the user features before the float32 rounding)."""
    user = np.asarray(cols.user).tolist()
    item = np.asarray(cols.item).tolist()
    rating = np.asarray(cols.rating, np.float32).astype(np.float64).tolist()
    votes = np.asarray(cols.helpful_vote).tolist()
    verified = np.asarray(cols.verified).astype(bool).tolist()
    stamp = np.asarray(cols.timestamp).tolist()
    n_rec = len(user)
    dated = ([True] * n_rec if cols.ts_valid is None
             else np.asarray(cols.ts_valid).astype(bool).tolist())
    words = np.asarray(cols.n_tokens).tolist()
    distinct = np.asarray(cols.n_unique_tokens).tolist()
    stars = [star(r) for r in rating]
    of_user, of_item = _filed(user), _filed(item)

    # per item: mean star (what a user's deviation is measured from), mean raw rating, count
    mean_star = {i: sum(stars[e] for e in recs) / len(recs) for i, recs in of_item.items()}
    item_x = np.zeros((num_items, 2), np.float32)
    for i, recs in of_item.items():
        item_x[i] = [sum(rating[e] for e in recs) / len(recs), len(recs)]

    avg_words = sum(words) / max(n_rec, 1)
    known = [stamp[e] for e in range(n_rec) if dated[e]]
    first, last = (min(known), max(known)) if known else (None, None)

    user_x64 = np.full((num_users, 7), math.nan)
    user_y = np.full(num_users, -1, np.int64)
    total_reviews = np.zeros(num_users, np.int32)
    helpful_reviews = np.zeros(num_users, np.int32)
    for u, recs in of_user.items():
        n = len(recs)
        n_helpful = sum(1 for e in recs if votes[e] > HELPFUL_ABOVE)
        ru = n_helpful / n
        hist = [sum(1 for e in recs if stars[e] == s) for s in (1, 2, 3, 4, 5)]
        entropy = 0.0
        for share in (c / n for c in hist if c):
            entropy -= share * math.log(share)
        days = [stamp[e] // TAU_MS for e in recs if dated[e]]     # floor division
        user_x64[u] = [
            ru,
            entropy,
            (hist[0] + hist[4]) / n,
            sum(abs(stars[e] - mean_star[item[e]]) for e in recs) / n,
            len(days) - len(set(days)),          # = sum over the days of (count - 1)
            sum(distinct[e] / words[e] for e in recs if words[e] > 0) / n,
            sum(abs(words[e] - avg_words) for e in recs) / n,
        ]
        user_y[u] = label_of(ru)
        total_reviews[u], helpful_reviews[u] = n, n_helpful

    edge_attr = np.empty((n_rec, 5), np.float32)
    for e in range(n_rec):
        align = 1.0 - abs(rating[e] - float(item_x[item[e], 0])) / 4.0
        when = (stamp[e] - first) / (last - first) if dated[e] and first != last else math.nan
        edge_attr[e] = [float(verified[e]), align, rating[e], when, float(votes[e])]

    return {
        "src": np.asarray(user, np.int32), "dst": np.asarray(item, np.int32),
        "edge_attr": edge_attr, "user_x": user_x64.astype(np.float32), "user_x64": user_x64,
        "user_y": user_y, "item_x": item_x, "total_reviews": total_reviews,
        "helpful_reviews": helpful_reviews,
        "stats": {"E": n_rec, "ts_min": first, "ts_max": last, "global_avg_len": avg_words},
    }
