"""Host restatement of the second feature pipeline (main_v2_.py:291-524, its
step 3) over review columns that carry their text: what
``bbgr.features.build_credibility_graph(.., feature_set="v2")`` computes.
Records are visited in file order and every per-record sum adds in that
order, in Python float (double), as the reference's two passes do; the gap
entropy goes through numpy exactly as the reference writes it (``np.diff``,
``np.floor(..).astype(int)``, ``np.clip``, ``np.unique(return_counts=True)``,
``-(p * np.log(p)).sum()``); the pooled distinct count is a ``set`` per user.
Everything that both pipelines share (labels, counts, ``item_x``,
``edge_attr``, user columns 0 to 2) comes from tests/features_ref.py.
The reference for tests/test_features_v2_host.py and
tests/test_gpu_features_v2.py. A helper, not a test module."""
import math
import types

import numpy as np

import features_ref as FR
import text_ref as TR

NEG_MAX_RATING = 2             # RNR counts the stars up to this
ETG_MAX_GAP_DAYS_CAP = 365
MS_FROM = 1_000_000_000_000    # a timestamp from here on is read as milliseconds


def record_tokens(text) -> list:
    """The token list of every record of a ``ReviewText`` (host arrays)."""
    data = np.asarray(text.data).tobytes()
    off = np.asarray(text.offsets).tolist()
    return [TR.regex_tokens(data[off[r]:off[r + 1]].decode("utf-8", "surrogatepass"))
            for r in range(len(off) - 1)]


def ts_to_days(ts_int: int) -> float:
    if ts_int >= MS_FROM:
        ts_int = ts_int / 1000.0
    return float(ts_int) / 86400.0


def entropy_from_counts_np(cnt: np.ndarray) -> float:
    s = float(cnt.sum())
    if s <= 0:
        return 0.0
    p = cnt[cnt > 0] / s
    return float(-(p * np.log(p)).sum())


def gap_bins(days: list) -> np.ndarray:
    """The capped whole-day bins of the gaps between the sorted times."""
    times = np.array(days, dtype=float)
    times = times[np.isfinite(times)]
    times.sort()
    gaps = np.diff(times)
    gaps = gaps[gaps >= 0]
    return np.clip(np.floor(gaps).astype(int), 0, ETG_MAX_GAP_DAYS_CAP)


def etg_of(days: list) -> float:
    if len(days) < 3:
        return 0.0
    bins = gap_bins(days)
    if bins.size == 0:
        return 0.0
    _, cnt = np.unique(bins, return_counts=True)
    return entropy_from_counts_np(cnt.astype(float))


def features_v2_ref(cols, num_users: int, num_items: int, tokens: list = None) -> dict:
    """Every output of the v2 build as numpy arrays, plus ``user_x64`` /
    ``user_extra64`` (before the float32 rounding), ``col6_sum`` (the per-user
    sum column 6 divides), ``pooled_tokens`` / ``pooled_unique`` per user and
    ``user_days``. ``tokens``: ``record_tokens(cols.text)`` if the caller has
    it already."""
    toks = record_tokens(cols.text) if tokens is None else tokens
    words = [len(t) for t in toks]
    shared = FR.features_ref(types.SimpleNamespace(
        user=cols.user, item=cols.item, rating=cols.rating, helpful_vote=cols.helpful_vote,
        verified=cols.verified, timestamp=cols.timestamp, ts_valid=cols.ts_valid,
        n_tokens=np.asarray(words, np.int32),
        n_unique_tokens=np.asarray([len(set(t)) for t in toks], np.int32)), num_users, num_items)
    user = np.asarray(cols.user).tolist()
    item = np.asarray(cols.item).tolist()
    rating = np.asarray(cols.rating, np.float32).astype(np.float64).tolist()
    stamp = np.asarray(cols.timestamp).tolist()
    n_rec = len(user)
    dated = ([True] * n_rec if cols.ts_valid is None
             else np.asarray(cols.ts_valid).astype(bool).tolist())

    # pass 1
    n_of, neg, tot_tokens, uniq, buckets, days = {}, {}, {}, {}, {}, {}
    item_sum, item_cnt = {}, {}
    lenlog_sum = 0.0
    for e in range(n_rec):
        u = user[e]
        n_of[u] = n_of.get(u, 0) + 1
        if FR.star(rating[e]) <= NEG_MAX_RATING:
            neg[u] = neg.get(u, 0) + 1
        item_sum[item[e]] = item_sum.get(item[e], 0.0) + rating[e]
        item_cnt[item[e]] = item_cnt.get(item[e], 0) + 1
        if words[e] > 0:
            tot_tokens[u] = tot_tokens.get(u, 0) + words[e]
            uniq.setdefault(u, set()).update(toks[e])
        lenlog_sum += math.log1p(words[e])
        if dated[e]:
            b = buckets.setdefault(u, {})
            b[stamp[e] // FR.TAU_MS] = b.get(stamp[e] // FR.TAU_MS, 0) + 1
            days.setdefault(u, []).append(ts_to_days(stamp[e]))
    item_mean = {k: item_sum[k] / item_cnt[k] for k in item_cnt}
    global_avg_lenlog = lenlog_sum / max(n_rec, 1)

    # pass 2
    ard_sum, rd_sum = {}, {}
    for e in range(n_rec):
        u = user[e]
        ard_sum[u] = ard_sum.get(u, 0.0) + abs(rating[e] - item_mean[item[e]])
        rd_sum[u] = rd_sum.get(u, 0.0) + abs(math.log1p(words[e]) - global_avg_lenlog)

    user_x64 = shared["user_x64"].copy()
    extra64 = np.full((num_users, 2), math.nan)
    col6_sum = np.zeros(num_users)
    pooled_tokens = np.zeros(num_users, np.int64)
    pooled_unique = np.zeros(num_users, np.int32)
    for u, n in n_of.items():
        burst = sum(max(c - 1, 0) for c in buckets.get(u, {}).values())
        tot, distinct = tot_tokens.get(u, 0), len(uniq.get(u, set()))
        user_x64[u, 3] = ard_sum[u] / n
        user_x64[u, 4] = burst / n
        user_x64[u, 5] = distinct / tot if tot > 0 else 0.0
        user_x64[u, 6] = rd_sum[u] / n
        extra64[u] = [neg.get(u, 0) / n, etg_of(days.get(u, []))]
        col6_sum[u] = rd_sum[u]
        pooled_tokens[u], pooled_unique[u] = tot, distinct

    out = dict(shared)
    out.update(user_x64=user_x64, user_x=user_x64.astype(np.float32), user_extra64=extra64,
               user_extra=extra64.astype(np.float32), col6_sum=col6_sum,
               pooled_tokens=pooled_tokens, pooled_unique=pooled_unique, user_days=days,
               stats=dict(shared["stats"], global_avg_lenlog=global_avg_lenlog))
    return out


# -- the corpus of tests/test_gpu_features_v2.py ------------------------------------------
U, I = 300, 200
HUB = 5500                     # records of the hub user (0) and of the hub item (0)
TS_COUNT_USERS = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4}    # user -> how many of its 6 records are dated
REPEAT_USER, EXACT_USER = 6, 10
EXACT_K = (1, 2, 3, 5, 7, 11, 30, 364)             # days between the two times of a pair
KELVIN_RECORDS = {20: 2, 21: 1}                    # user -> records that hold U+212A
_SEPS = [" ", " ", " ", ", ", ". ", "''", " '", "' ", "-", "\n", " é ", " İ", "’", " 😀 ", " "]


def _vocabulary() -> list:
    """About 2,000 distinct tokens: plain words and some with an apostrophe part."""
    vocab = [TR.word(k) for k in range(1900)]
    vocab += [TR.word(k) + "'" + TR.word(k % 7) for k in range(0, 1900, 19)]
    return vocab


def _exact_pairs(rng) -> list:
    """Pairs (t, t + k * 86 400 000) of millisecond times at large offsets,
    400 days apart from each other: the floor of the difference of the two
    doubles lands on k or on k - 1, as their roundings decide."""
    out = []
    for j, k in enumerate(EXACT_K):
        t = 1_500_000_000_000 + j * 400 * FR.TAU_MS + int(rng.integers(0, FR.TAU_MS))
        out += [t, t + k * FR.TAU_MS]
    return out


_corpus_cache = []


def gpu_corpus() -> dict:
    """Columns (numpy, file order shuffled) and ``records`` (the strings) of
    the case tests/test_gpu_features_v2.py runs and
    tests/test_features_v2_host.py checks on the host. Built once."""
    if _corpus_cache:
        return _corpus_cache[0]
    rng = np.random.default_rng(2025)
    n_base = 8600
    user = [rng.integers(7, U - 1, n_base)]                 # user U - 1 has no record
    item = [rng.integers(1, I - 1, n_base)]                 # item I - 1 has no record
    user.append(np.zeros(HUB, np.int64))                    # the hub user
    item.append(rng.integers(0, I - 1, HUB))
    user.append(rng.integers(7, U - 1, HUB))                # the hub item
    item.append(np.zeros(HUB, np.int64))
    for u in list(TS_COUNT_USERS) + [REPEAT_USER]:
        user.append(np.full(6, u))
        item.append(rng.integers(1, I - 1, 6))
    user, item = np.concatenate(user), np.concatenate(item)
    E = user.size
    rating = rng.choice(np.array([0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 7]), E)
    helpful = rng.choice(np.array([0, 0, 0, 1, 5, 6, 7, 20]), E)
    verified = rng.uniform(size=E) < 0.5

    # timestamps: milliseconds (>= 10^12), seconds, a few negative; 10 % absent
    ts = 1_200_000_000_000 + rng.integers(0, 3000 * FR.TAU_MS, E)
    secs = rng.uniform(size=E) < 0.25
    ts[secs] = 1_000_000_000 + rng.integers(0, 3000 * 86_400, int(secs.sum()))
    neg = rng.uniform(size=E) < 0.02
    ts[neg] = -rng.integers(1, 5 * FR.TAU_MS, int(neg.sum()))
    ts_valid = rng.uniform(size=E) >= 0.1
    hub = np.flatnonzero(user == 0)
    # the hub user's times by their gaps: whole days 0 .. 399 in turn (all 366 bins, and the
    # cap) plus a part of a day; every 7th gap exactly 0 (a repeated timestamp)
    gap = (np.arange(hub.size) % 400) * FR.TAU_MS + rng.integers(0, FR.TAU_MS, hub.size)
    gap[::7] = 0
    ts[hub] = 1_200_000_000_000 + np.cumsum(gap)
    for u, k in TS_COUNT_USERS.items():
        rec = np.flatnonzero(user == u)
        ts_valid[rec] = np.arange(rec.size) < k
    rec = np.flatnonzero(user == REPEAT_USER)
    ts[rec], ts_valid[rec] = 1_300_000_000_777, True
    rec = np.flatnonzero(user == EXACT_USER)
    pairs = _exact_pairs(rng)
    assert rec.size >= len(pairs)
    ts[rec[:len(pairs)]], ts_valid[rec[:len(pairs)]] = pairs, True
    ts_valid[rec[len(pairs):]] = False

    # text: 0 - 60 words of the user's own window of the vocabulary, in mixed case
    vocab = _vocabulary()
    records = []
    for e in range(E):
        if rng.uniform() < 0.1:
            records.append("")
            continue
        lo = int(user[e]) * 37 % (len(vocab) - 120)
        parts = []
        for k in rng.integers(lo, lo + 120, int(rng.integers(0, 61))).tolist():
            w = vocab[k]
            parts.append((w, w, w.upper(), w.capitalize())[int(rng.integers(0, 4))])
            parts.append(_SEPS[int(rng.integers(0, len(_SEPS)))])
        records.append("".join(parts))
    for u, k in KELVIN_RECORDS.items():
        for e in np.flatnonzero(user == u)[:k].tolist():
            records[e] = records[e] + " Kelvin k K"
    order = rng.permutation(E)                              # file order mixes all of it
    corpus = dict(
        user=user[order].astype(np.int32), item=item[order].astype(np.int32),
        rating=rating[order].astype(np.float32), helpful_vote=helpful[order].astype(np.int32),
        verified=verified[order].astype(np.uint8), timestamp=ts[order].astype(np.int64),
        ts_valid=ts_valid[order], records=[records[e] for e in order.tolist()])
    _corpus_cache.append(corpus)
    return corpus


def text_of(records: list):
    """(data uint8, offsets int64 [n + 1]) of the records' UTF-8 bytes."""
    enc = [TR.encode(s) for s in records]
    offsets = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum([len(b) for b in enc], out=offsets[1:])
    return np.frombuffer(bytearray().join(enc), np.uint8), offsets


def corpus_columns(corpus: dict):
    """The corpus as the attribute bag features_v2_ref reads (``text`` with
    ``data`` and ``offsets``; no token columns)."""
    data, offsets = text_of(corpus["records"])
    return types.SimpleNamespace(
        **{k: v for k, v in corpus.items() if k != "records"},
        text=types.SimpleNamespace(data=data, offsets=offsets))
