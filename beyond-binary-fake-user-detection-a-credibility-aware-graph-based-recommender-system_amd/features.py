"""Review columns -> the credibility graph's tensors, on the device.

Restates the numeric part of main.py:153-606: the Ru label per user (step 1,
:153-196), the six behavioural features per user (step 3, :247-373) and the
graph pass (:423-570): ``user_x [U, 7]``, ``user_y [U]``, ``item_x [I, 2]``,
``edge_attr [E, 5]``. Their output is what ``cred_train.SlasGraph`` takes::

    cols, user2idx, item2idx = review_columns_from_jsonl("reviews.jsonl")
    out = build_credibility_graph(cols, len(user2idx), len(item2idx), device="cuda")
    g = SlasGraph((out.src, out.dst), out.edge_attr, out.user_x, out.user_y, out.item_x, "cuda")

The device part starts at numeric per-review columns; the string work (JSON,
id -> index maps) is the one host pass of ``review_columns_from_jsonl``. The
tokeniser runs in that pass by default (``tokens="host"``) or on the device
(``tokens="device"``: the pass collects the encoded text and ``bbgr.text``
counts the tokens; the columns are the same integers either way).

A record is a review that has a user, an item and a rating: the records steps
3 and 5 of the reference keep. Step 1 of the reference also counts, in
``total_reviews`` and so in Ru, the reviews of a user that lack an item or a
rating; this interface does not see them. A missing ``helpful_vote`` is 0 (the
reference's label pass reads it so; its edge attribute would be NaN). Ratings
are finite, and timestamps span less than 2^53 ms (the normalised timestamp
divides exact doubles; a wider span is a ValueError).

Launches of one call: ``bbgr_feat_stats`` (one host read of four integers),
``bbgr_feat_buckets``, three ``bbgr_csr_build`` (records by user and by item,
keyed by the id alone, and (user, day bucket) sorted), ``bbgr_feat_items``, ``bbgr_feat_users``,
``bbgr_feat_edges``. All sums run in double in a fixed order without float
atomics: two calls give the same bits.

``feature_set="v2"`` builds the later pipeline, main_v2_.py:291-524, for the
same graph pass and model: columns 3 to 6 in its definitions (deviation from
the item mean of the raw rating, the burst count over n, POOLED lexical
diversity, the discrepancy of ``log1p`` lengths) and ``user_extra`` = (RNR,
ETG) beside them. It needs ``cols.text`` (``bbgr.text.pooled_token_counts``:
by default resident as one chunk, below 2^31 - 1 bytes; with
``text_chunk_bytes`` of any size that fits the device beside one chunk,
regrouped by user with ``bbgr_text_gather`` into chunks of whole users, the
same bits; users it flags are counted again on the host) and adds
``bbgr_feat_lenlog``, ``bbgr_feat_item_means``, ``bbgr_text_unique_pooled``,
``bbgr_feat_gaps`` and ``bbgr_feat_users_v2`` in ``bbgr_feat_users``' place.
"""
from __future__ import annotations

import ctypes
import dataclasses
import json
import re
from dataclasses import dataclass
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_handle

# main.py:71-84
EDGE_ATTR_KEYS = ["verified", "rating_align", "rating", "timestamp_norm", "helpful_vote"]
USER_FEATURE_KEYS = ["Ru", "rating_entropy", "extremity_ratio", "average_rating_deviation",
                     "review_burst_count", "lexical_diversity", "review_length_discrepancy"]
USER_EXTRA_KEYS = ["RNR", "ETG"]    # main_v2_.py:491-508, beside the seven
FEATURE_SETS = ("main", "v2")
TAU_MS = 24 * 60 * 60 * 1000


class _UnsetIsAbsent:
    """The field ``ReviewColumns.text``: None by default, and kept out of the
    instance's ``__dict__`` while it is None, so that callers who walk the
    columns through ``cols.__dict__`` still meet arrays only."""

    def __get__(self, obj, owner=None):
        return None if obj is None else obj.__dict__.get("text")

    def __set__(self, obj, value):
        if value is None:
            obj.__dict__.pop("text", None)
        else:
            obj.__dict__["text"] = value


@dataclass
class ReviewColumns:
    """One entry per record, in file order (numpy arrays, memory maps or
    tensors). ``user`` / ``item``: int32 ids as the caller's maps assign them;
    ``rating`` float32; ``helpful_vote`` int32; ``verified`` uint8 / bool;
    ``timestamp`` int64 milliseconds, ``ts_valid`` an optional mask (False: the
    record has no timestamp; None: every record has one); ``n_tokens`` =
    len(tokenize(title + " " + text)) and ``n_unique_tokens`` = len(set(..)),
    int32, or both None and ``text`` the records' bytes (``bbgr.text.ReviewText``),
    from which ``build_credibility_graph`` counts them on the device."""
    user: Any
    item: Any
    rating: Any
    helpful_vote: Any
    verified: Any
    timestamp: Any
    n_tokens: Any = None
    n_unique_tokens: Any = None
    ts_valid: Any = None
    text: Any = _UnsetIsAbsent()

    def __len__(self) -> int:
        return int(self.user.shape[0])


class CredibilityGraph(NamedTuple):
    """Device tensors of ``build_credibility_graph``; ``stats`` is a host dict."""
    src: torch.Tensor               # int32 [E]
    dst: torch.Tensor               # int32 [E]
    edge_attr: torch.Tensor         # f32 [E, 5], EDGE_ATTR_KEYS
    user_x: torch.Tensor            # f32 [U, 7], USER_FEATURE_KEYS
    user_y: torch.Tensor            # int64 [U]: 1 genuine, 0 fake, -1 unlabeled
    item_x: torch.Tensor            # f32 [I, 2]: mean raw rating, count
    total_reviews: torch.Tensor     # int32 [U]
    helpful_reviews: torch.Tensor   # int32 [U]
    stats: dict                     # E, ts_min, ts_max (None without timestamps), global_avg_len


class CredibilityGraphV2(NamedTuple):
    """``build_credibility_graph(.., feature_set="v2")``: the fields of
    ``CredibilityGraph`` (``user_x`` in main_v2_.py's definitions, ``stats``
    with ``global_avg_lenlog``), then ``user_extra``."""
    src: torch.Tensor
    dst: torch.Tensor
    edge_attr: torch.Tensor
    user_x: torch.Tensor
    user_y: torch.Tensor
    item_x: torch.Tensor
    total_reviews: torch.Tensor
    helpful_reviews: torch.Tensor
    stats: dict
    user_extra: torch.Tensor        # f32 [U, 2], USER_EXTRA_KEYS


def _column(x, name: str, E: int, device, dtype) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=dtype).contiguous()
    else:
        a = np.ascontiguousarray(np.asarray(x))
        t = torch.from_numpy(a).to(device=device, dtype=dtype).contiguous()
    if t.dim() != 1 or t.numel() != E:
        raise ValueError(f"column {name}: expected {E} entries, got shape {tuple(t.shape)}")
    return t


def _id_range(x) -> tuple[int, int]:
    """(min, max) of an id column: on the host for host columns."""
    if isinstance(x, torch.Tensor):
        lo, hi = torch.aminmax(x)
        return int(lo), int(hi)
    a = np.asarray(x)
    return int(a.min()), int(a.max())


def _check_ids(x, name: str, bound: int, what: str) -> None:
    lo, hi = _id_range(x)
    if lo < 0 or hi >= bound:
        raise ValueError(f"{name} id out of range: [{lo}, {hi}] not within [0, {what} = {bound})")


def _csr_build(rows: torch.Tensor, cols: torch.Tensor, n_rows: int, n_cols: int, perm=None):
    """(indptr int32 [n_rows + 1], indices int32 [E]) of bbgr_csr_build: rows
    ascending, columns ascending within a row, equal pairs in input order;
    `perm` (int32 [E], optional) receives the input position of every slot."""
    dev = rows.device
    E = rows.numel()
    indptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    indices = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    _lib.call_with_workspace("bbgr_csr_build", E, ptr(rows), ptr(cols), n_rows, n_cols,
                             ptr(indptr), ptr(indices), ptr(perm), device=dev)
    return indptr, indices


def _group(ids: torch.Tensor, zeros: torch.Tensor, n_rows: int):
    """The reference-order rows of an id column: (indptr, record ids), a row's
    records ascending. The sort key is the id alone (one column of zeros): the
    build is stable, so its permutation lists each row in file order."""
    eid = torch.empty(max(ids.numel(), 1), dtype=torch.int32, device=ids.device)
    indptr, _ = _csr_build(ids, zeros, n_rows, 1, perm=eid)
    return indptr, eid


def build_credibility_graph(cols: ReviewColumns, num_users: int, num_items: int,
                            device="cuda", feature_set: str = "main", text_chunk_bytes=None):
    """Labels, user and item features and edge attributes of the records in
    `cols` (module docstring). Raises ValueError, before any launch, for an id
    outside [0, num_users) / [0, num_items) or E >= 2^31 - 1, and
    ``_lib.BbgrError`` (BBGR_ERR_INVALID, naming timestamp) when the day
    buckets of the smallest and largest timestamp are 2^31 - 1 or more apart;
    ValueError naming timestamp when they span 2^53 ms or more.
    A user id with no record gets a NaN row of ``user_x`` and label -1; an
    item id with no record mean 0 and count 0. Without the two token columns
    they are counted from ``cols.text`` (``bbgr.text.token_counts``); ValueError
    when neither is given or ``text`` has another number of records.
    ``feature_set="main"`` returns a ``CredibilityGraph``; ``"v2"`` (module
    docstring) a ``CredibilityGraphV2`` and needs ``cols.text``: ValueError
    naming text without it, or for text of 2^31 - 1 bytes or more; ``n_tokens``
    is taken from the columns when given, else counted.
    ``text_chunk_bytes=<int>`` ("v2"; accepted and unused by "main") lifts that
    limit: the text goes to the device once, ``token_counts`` and the pooled
    count both read it there, and the pooled count regroups it by user into
    chunks of at most that many bytes (``pooled_token_counts(.., chunk_bytes)``)
    over the user rows this build groups anyway. The same tensors come back.
    A record and a user's text stay below 2^31 - 1 bytes each."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("build_credibility_graph runs on the GPU; there is no CPU fallback")
    if feature_set not in FEATURE_SETS:
        raise ValueError(f"feature_set = {feature_set!r}: one of {FEATURE_SETS}")
    U, I, E = int(num_users), int(num_items), len(cols)
    v2 = feature_set == "v2"
    if v2:
        from .text import BYTES_MAX
        if cols.text is None:
            raise ValueError("feature_set='v2' needs cols.text: the pooled distinct-token count "
                             "cannot be made from two integers per record")
        if len(cols.text) != E:
            raise ValueError(f"text: expected {E} records, got {len(cols.text)}")
        if text_chunk_bytes is not None and int(text_chunk_bytes) < 1:
            raise ValueError("text_chunk_bytes must be at least 1")
        span = int(cols.text.offsets[-1]) - int(cols.text.offsets[0])
        if text_chunk_bytes is None and span >= BYTES_MAX:
            raise ValueError(f"text of {span} bytes: feature_set='v2' takes the text as one "
                             "chunk, which must be shorter than 2^31 - 1 bytes")
    elif cols.n_tokens is None or cols.n_unique_tokens is None:
        if cols.text is None:
            raise ValueError("columns n_tokens / n_unique_tokens: give both, or text")
        if len(cols.text) != E:
            raise ValueError(f"text: expected {E} records, got {len(cols.text)}")
    if U < 0 or I < 0 or U >= 2**31 - 1 or I >= 2**31 - 1:
        raise ValueError("num_users and num_items must lie in [0, 2^31 - 1)")
    if E >= 2**31 - 1:
        raise ValueError(f"E = {E} records: E must be < 2^31 - 1")
    if E:
        _check_ids(cols.user, "user", U, "num_users")
        _check_ids(cols.item, "item", I, "num_items")
    _lib.require_gpu()
    if v2 and text_chunk_bytes is not None:
        from .text import resident
        cols = dataclasses.replace(cols, text=resident(cols.text, device))   # the one upload
    if v2 and cols.n_tokens is not None:
        if cols.n_unique_tokens is None:     # not read by the v2 pass; the columns struct wants one
            cols = dataclasses.replace(cols, n_unique_tokens=cols.n_tokens)
    elif cols.n_tokens is None or cols.n_unique_tokens is None:
        from .text import token_counts
        n_tok, n_uniq, _ = token_counts(cols.text, device)
        cols = dataclasses.replace(cols, n_tokens=n_tok, n_unique_tokens=n_uniq)
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        if not v2:
            return _Pipeline(cols, U, I, E, dev).run()
        return _PipelineV2(cols, U, I, E, dev, text_chunk_bytes).run()


class _Pipeline:
    """The launches of one build, one method each (tools/features_bench.py
    times them one by one); `run` is their order."""

    def __init__(self, cols: ReviewColumns, U: int, I: int, E: int, dev):
        self.U, self.I, self.E, self.dev = U, I, E, dev
        self.user = _column(cols.user, "user", E, dev, torch.int32)
        self.item = _column(cols.item, "item", E, dev, torch.int32)
        self.rating = _column(cols.rating, "rating", E, dev, torch.float32)
        self.helpful = _column(cols.helpful_vote, "helpful_vote", E, dev, torch.int32)
        self.verified = _column(cols.verified, "verified", E, dev, torch.uint8)
        self.ts = _column(cols.timestamp, "timestamp", E, dev, torch.int64)
        self.ts_valid = (None if cols.ts_valid is None else
                         _column(cols.ts_valid, "ts_valid", E, dev, torch.bool).view(torch.uint8))
        self.n_tok = _column(cols.n_tokens, "n_tokens", E, dev, torch.int32)
        self.n_uniq = _column(cols.n_unique_tokens, "n_unique_tokens", E, dev, torch.int32)
        c = self.c = _lib.FeatColumns()
        c.n, c.n_users, c.n_items = E, U, I
        c.user, c.item, c.rating = ptr(self.user), ptr(self.item), ptr(self.rating)
        c.helpful_vote, c.verified = ptr(self.helpful), ptr(self.verified)
        c.timestamp, c.ts_valid = ptr(self.ts), ptr(self.ts_valid)
        c.n_tokens, c.n_unique_tokens = ptr(self.n_tok), ptr(self.n_uniq)
        self.cref = ctypes.byref(c)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        self.stats_dev = torch.empty(4, dtype=torch.int64, device=dev)
        self.rows_b = torch.empty(max(E, 1), **i32)
        self.cols_b = torch.empty(max(E, 1), **i32)
        self.zeros = torch.zeros(max(E, 1), **i32)
        self.item_x = torch.empty(I, 2, **f32)
        self.item_rbar = torch.empty(max(I, 1), dtype=torch.float64, device=dev)
        self.user_x = torch.empty(U, 7, **f32)
        self.user_y = torch.empty(U, dtype=torch.int64, device=dev)
        self.total = torch.empty(U, **i32)
        self.helpful_reviews = torch.empty(U, **i32)
        self.edge_attr = torch.empty(E, len(EDGE_ATTR_KEYS), **f32)

    def stats(self) -> None:
        call("bbgr_feat_stats", self.cref, ptr(self.stats_dev), stream_handle())

    def read_stats(self) -> None:
        """The one host read: four integers."""
        self.ts_min, self.ts_max, self.n_ts, len_sum = (int(v) for v in self.stats_dev.tolist())
        self.global_avg_len = len_sum / max(self.E, 1)

    def buckets(self) -> None:
        n_cols = ctypes.c_int32(0)
        call("bbgr_feat_buckets", self.cref, self.ts_min, self.ts_max, ptr(self.rows_b),
             ptr(self.cols_b), ctypes.byref(n_cols), stream_handle())
        self.n_bucket_cols = n_cols.value
        if self.n_ts and self.ts_max - self.ts_min >= 2**53:
            raise ValueError(f"timestamp: ts_max - ts_min = {self.ts_max - self.ts_min} ms; the "
                             "span must be < 2^53 (timestamp_norm divides exact doubles)")

    def group_users(self) -> None:
        self.u_indptr, self.u_eid = _group(self.user, self.zeros, self.U)

    def group_items(self) -> None:
        self.i_indptr, self.i_eid = _group(self.item, self.zeros, self.I)

    def group_buckets(self) -> None:
        E = self.E
        self.b_indptr, self.b_bucket = _csr_build(self.rows_b[:E], self.cols_b[:E], self.U + 1,
                                                  self.n_bucket_cols)

    def items(self) -> None:
        _lib.call_with_workspace("bbgr_feat_items", self.cref, ptr(self.i_indptr),
                                 ptr(self.i_eid), ptr(self.item_x), ptr(self.item_rbar),
                                 device=self.dev)

    def users(self) -> None:
        a = _lib.FeatUserArgs()
        a.u_indptr, a.u_eid = ptr(self.u_indptr), ptr(self.u_eid)
        a.b_indptr, a.b_bucket = ptr(self.b_indptr), ptr(self.b_bucket)
        a.item_rbar, a.global_avg_len = ptr(self.item_rbar), self.global_avg_len
        a.user_x, a.user_y = ptr(self.user_x), ptr(self.user_y)
        a.total_reviews, a.helpful_reviews = ptr(self.total), ptr(self.helpful_reviews)
        _lib.call_with_workspace("bbgr_feat_users", self.cref, ctypes.byref(a), device=self.dev)

    def edges(self) -> None:
        call("bbgr_feat_edges", self.cref, ptr(self.item_x), self.ts_min, self.ts_max,
             ptr(self.edge_attr), stream_handle())

    STEPS = ("stats", "read_stats", "buckets", "group_users", "group_items", "group_buckets",
             "items", "users", "edges")

    def run(self) -> CredibilityGraph:
        for step in self.STEPS:
            getattr(self, step)()
        has_ts = self.n_ts > 0
        stats = {"E": self.E, "ts_min": self.ts_min if has_ts else None,
                 "ts_max": self.ts_max if has_ts else None,
                 "global_avg_len": self.global_avg_len}
        return CredibilityGraph(self.user, self.item, self.edge_attr, self.user_x, self.user_y,
                                self.item_x, self.total, self.helpful_reviews, stats)


class _PipelineV2(_Pipeline):
    """The v2 build: `_Pipeline`'s launches with the v2 statistics beside
    them, the pooled count and the gap entropy before the user pass, and
    ``bbgr_feat_users_v2`` as the user pass."""

    def __init__(self, cols: ReviewColumns, U: int, I: int, E: int, dev, text_chunk_bytes=None):
        super().__init__(cols, U, I, E, dev)
        self.text = cols.text
        self.text_chunk_bytes = text_chunk_bytes
        f64 = dict(dtype=torch.float64, device=dev)
        self.lenlog_dev = torch.empty(1, **f64)
        self.item_mean = torch.empty(max(I, 1), **f64)
        self.etg = torch.empty(max(U, 1), **f64)
        self.user_extra = torch.empty(U, len(USER_EXTRA_KEYS), dtype=torch.float32, device=dev)

    def stats(self) -> None:
        super().stats()
        _lib.call_with_workspace("bbgr_feat_lenlog", self.cref, ptr(self.lenlog_dev),
                                 device=self.dev)

    def read_stats(self) -> None:
        """The one host read: four integers and the sum of log1p(n_tokens)."""
        super().read_stats()
        self.global_avg_lenlog = float(self.lenlog_dev) / max(self.E, 1)

    def items(self) -> None:
        super().items()
        _lib.call_with_workspace("bbgr_feat_item_means", self.cref, ptr(self.i_indptr),
                                 ptr(self.i_eid), ptr(self.item_mean), device=self.dev)

    def pooled(self) -> None:
        from .text import pooled_token_counts
        if self.text_chunk_bytes is None:
            self.group_tokens, self.group_unique, self.pooled_info = pooled_token_counts(
                self.text, self.user, self.U, self.dev)
            return
        # regrouped by user, over the user rows group_users has built
        self.group_tokens, self.group_unique, self.pooled_info = pooled_token_counts(
            self.text, self.user, self.U, self.dev, chunk_bytes=self.text_chunk_bytes,
            group_csr=(self.u_indptr, self.u_eid))

    def gaps(self) -> None:
        _lib.call_with_workspace("bbgr_feat_gaps", self.cref, ptr(self.u_indptr),
                                 ptr(self.u_eid), ptr(self.etg), device=self.dev)

    def users(self) -> None:
        a = _lib.FeatUserV2Args()
        a.u_indptr, a.u_eid = ptr(self.u_indptr), ptr(self.u_eid)
        a.b_indptr, a.b_bucket = ptr(self.b_indptr), ptr(self.b_bucket)
        a.item_mean, a.global_avg_lenlog = ptr(self.item_mean), self.global_avg_lenlog
        a.group_tokens, a.group_unique = ptr(self.group_tokens), ptr(self.group_unique)
        a.etg = ptr(self.etg)
        a.user_x, a.user_y = ptr(self.user_x), ptr(self.user_y)
        a.total_reviews, a.helpful_reviews = ptr(self.total), ptr(self.helpful_reviews)
        a.user_extra = ptr(self.user_extra)
        _lib.call_with_workspace("bbgr_feat_users_v2", self.cref, ctypes.byref(a),
                                 device=self.dev)

    STEPS = ("stats", "read_stats", "buckets", "group_users", "group_items", "group_buckets",
             "items", "pooled", "gaps", "users", "edges")

    def run(self) -> CredibilityGraphV2:
        g = super().run()
        g.stats["global_avg_lenlog"] = self.global_avg_lenlog
        return CredibilityGraphV2(*g, self.user_extra)


# -- the host reader -------------------------------------------------------------------
# lower-case runs of ASCII letters, optionally one apostrophe part inside
_TOKEN = re.compile(r"[a-z]+(?:'[a-z]+)?")


def tokenize(text: str) -> list:
    return _TOKEN.findall(text.lower()) if text else []


def _as_int(x):
    try:
        return int(x)
    except (TypeError, ValueError, OverflowError):
        return None


def review_columns_from_jsonl(path, item_id_key: str = "parent_asin", tokens: str = "host",
                              device="cuda"):
    """One streaming pass over a review dump (one JSON object per line) ->
    ``(ReviewColumns, user2idx, item2idx)``. Records without a ``user_id``, an
    item id or a ``rating`` are skipped; ids are assigned in order of first
    appearance among the kept records, as the reference's graph pass does.
    ``tokens="host"`` tokenises every record in the pass; ``tokens="device"``
    only encodes it and counts the tokens of all records on ``device``
    afterwards (``bbgr.text.token_counts``): the same two columns, as device
    tensors, and the bytes themselves in ``cols.text``."""
    if tokens not in ("host", "device"):
        raise ValueError(f"tokens = {tokens!r}: 'host' or 'device'")
    on_device = tokens == "device"
    encoded: list = []
    user2idx: dict = {}
    item2idx: dict = {}
    user, item, rating, helpful, verified, ts, ts_valid, n_tok, n_uniq = ([] for _ in range(9))
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for line in f:
            if not line.strip():
                continue
            r = json.loads(line)
            uid, iid, rt = r.get("user_id"), r.get(item_id_key), r.get("rating")
            if rt is None or not (uid and iid):
                continue
            user.append(user2idx.setdefault(uid, len(user2idx)))
            item.append(item2idx.setdefault(iid, len(item2idx)))
            rating.append(float(rt))
            helpful.append(_as_int(r.get("helpful_vote", 0)) or 0)
            verified.append(bool(r.get("verified_purchase", False)))
            t = _as_int(r.get("timestamp"))
            ts.append(0 if t is None else t)
            ts_valid.append(t is not None)
            s = " ".join((r.get("title") or "", r.get("text") or ""))
            if on_device:
                encoded.append(s.encode("utf-8", "surrogatepass"))
                continue
            toks = tokenize(s)
            n_tok.append(len(toks))
            n_uniq.append(len(set(toks)))
    text = None
    if on_device:
        from .text import ReviewText, token_counts
        text = ReviewText.from_encoded(encoded)
        n_tok, n_uniq, _ = token_counts(text, device)
    cols = ReviewColumns(
        user=np.asarray(user, np.int32), item=np.asarray(item, np.int32),
        rating=np.asarray(rating, np.float32), helpful_vote=np.asarray(helpful, np.int32),
        verified=np.asarray(verified, np.uint8), timestamp=np.asarray(ts, np.int64),
        n_tokens=n_tok if on_device else np.asarray(n_tok, np.int32),
        n_unique_tokens=n_uniq if on_device else np.asarray(n_uniq, np.int32),
        ts_valid=np.asarray(ts_valid, np.bool_), text=text)
    return cols, user2idx, item2idx
