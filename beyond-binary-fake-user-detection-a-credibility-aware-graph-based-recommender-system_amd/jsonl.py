"""The review dump -> columns, text and id tables, parsed on the device.

``features.review_columns_from_jsonl`` over the file's bytes::

    parsed = read_reviews("reviews.jsonl")           # a path, bytes, a uint8 array or tensor
    out = build_credibility_graph(parsed.cols, len(parsed.user_ids), len(parsed.item_ids))
    split = split_interactions(parsed.cols.user, parsed.cols.item, parsed.cols.rating,
                               parsed.user_ids, parsed.item_ids)
    user2idx = id_dict(parsed.user_ids)              # the reader's dict, only when asked for

For every file whose lines ``json.loads`` accepts the result equals, bit for
bit, ``review_columns_from_jsonl(path, item_id_key, tokens="device")``: every
column, ``cols.text``, and the id tables of ``user2idx`` / ``item2idx`` (ids
encoded ``surrogatepass``).

The rule (include/bbgr.h spells it out): ``\\n`` and ``\\r`` end a
line, a line of spaces and tabs is blank, a ``:`` at bracket depth 1 outside
strings ends a top-level key, the last occurrence of a key wins. The device
vouches for the value forms real dumps consist of and flags every other line;
a flagged line is parsed here with the host reader's own expressions
(``host_record``), so an unflagged line is exact, not merely probable, and a
flagged line that makes the host reader raise raises the same exception type
here. Two differences: malformed JSON that no value read depends on (such as
``"images": [tru]``) is not detected as long as strings and brackets balance;
and an id that is truthy and hashable but not a string (``"user_id": 5``),
which the host reader keeps as a dict key, is a TypeError here.

Per chunk (line-aligned, at most ``chunk_bytes``): ``bbgr_jsonl_count`` (one
host read: the lines), ``bbgr_jsonl_lines``, ``bbgr_jsonl_scan`` (one host
read: the four line counts), the host pass over flagged lines if there are
any, ``bbgr_jsonl_offsets`` (one host read: the four totals),
``bbgr_jsonl_write``. After the last chunk ``bbgr_ids_number`` and
``bbgr_ids_table`` per side (first-appearance numbering by hash, sort and
byte comparison; a hash collision between different strings numbers that side
on the host instead and is reported), then ``bbgr.text.token_counts``.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_handle
from .features import ReviewColumns, _as_int
from .split import IdTable
from .text import ReviewText, token_counts

BYTES_MAX = 2**31 - 1      # a chunk's bytes, and so a line's, stay below this
KEY_MAX = 255              # bytes of item_id_key
_SEARCH = 1 << 20          # bytes the planner looks at per step
BLANK, SKIPPED, KEPT, FLAGGED, HOST = range(5)   # line status (include/bbgr.h)


class ParsedReviews(NamedTuple):
    cols: ReviewColumns     # device tensors; cols.text a device-resident ReviewText
    user_ids: IdTable       # device tensors, id order
    item_ids: IdTable
    info: dict              # lines, records, blank, skipped, flagged, numbering_fallback
                            # (sides numbered on the host), chunks: host ints


def id_dict(table: IdTable) -> dict:
    """``{id string: index}`` of an id table: the reader's ``user2idx``."""
    data = table.data.cpu().numpy() if isinstance(table.data, torch.Tensor) else np.asarray(table.data)
    off = (table.offsets.cpu().numpy() if isinstance(table.offsets, torch.Tensor)
           else np.asarray(table.offsets)).tolist()
    raw = data.tobytes()
    return {raw[off[k]:off[k + 1]].decode("utf-8", "surrogatepass"): k
            for k in range(len(off) - 1)}


def _key_bytes(item_id_key) -> bytes:
    if not isinstance(item_id_key, str) or not item_id_key:
        raise ValueError("item_id_key must be a non-empty str")
    if any(ord(c) < 0x20 or ord(c) > 0x7E or c in '"\\' for c in item_id_key):
        raise ValueError(f"item_id_key = {item_id_key!r}: ASCII without quote, backslash or "
                         "control bytes")
    if len(item_id_key) > KEY_MAX:
        raise ValueError(f"item_id_key of {len(item_id_key)} bytes: at most {KEY_MAX}")
    return item_id_key.encode("ascii")


def _source(src):
    """A host uint8 array (a memory map for a path) or a uint8 device tensor."""
    if isinstance(src, (str, os.PathLike)):
        if os.path.getsize(src) == 0:
            return np.zeros(0, np.uint8)
        return np.memmap(src, np.uint8, "r")
    if isinstance(src, (bytes, bytearray, memoryview)):
        return np.frombuffer(src, np.uint8)
    if isinstance(src, torch.Tensor):
        if src.dtype != torch.uint8 or src.dim() != 1:
            raise ValueError("src: a uint8 vector")
        return src.contiguous() if src.is_cuda else src.contiguous().numpy()
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("src: a path, bytes, or a uint8 vector")
    return a


def _host_bytes(data, b0: int, b1: int) -> np.ndarray:
    a = data[b0:b1]
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _last_terminator(data, lo: int, hi: int) -> int:
    """The last position in [lo, hi) that holds ``\\n`` or ``\\r``, or -1."""
    while hi > lo:
        at = max(lo, hi - _SEARCH)
        blk = _host_bytes(data, at, hi)
        hit = np.flatnonzero((blk == 10) | (blk == 13))
        if hit.size:
            return at + int(hit[-1])
        hi = at
    return -1


def _next_terminator(data, lo: int, n: int) -> int:
    """The first position in [lo, n) that holds a terminator, or n."""
    while lo < n:
        blk = _host_bytes(data, lo, min(n, lo + _SEARCH))
        hit = np.flatnonzero((blk == 10) | (blk == 13))
        if hit.size:
            return lo + int(hit[0])
        lo += blk.shape[0]
    return n


def _cut(data, b0: int, chunk_bytes: int) -> int:
    """Where the chunk that starts at b0 ends: after the last line terminator
    within ``chunk_bytes``; a line longer than that is a chunk of its own, up
    to its terminator. ValueError for a chunk of ``BYTES_MAX`` bytes or more:
    a line that long."""
    n = int(data.shape[0])
    if n - b0 <= chunk_bytes:
        b1 = n
    else:
        cut = _last_terminator(data, b0, b0 + chunk_bytes)
        b1 = cut + 1 if cut >= 0 else min(_next_terminator(data, b0 + chunk_bytes, n) + 1, n)
    if b1 - b0 >= BYTES_MAX:
        raise ValueError(f"the line at byte {b0} has {b1 - b0} bytes or more: a line must be "
                         f"shorter than {BYTES_MAX} bytes")
    return b1


def _chunk_bytes(chunk_bytes) -> int:
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be at least 1")
    return min(chunk_bytes, BYTES_MAX - 1)


def plan_chunks(data, chunk_bytes: int) -> list:
    """[(b0, b1), ..]: the consecutive line-aligned byte ranges ``read_reviews``
    uploads one by one (``_cut``); they cover ``data``."""
    chunk_bytes = _chunk_bytes(chunk_bytes)
    chunks, b0 = [], 0
    while b0 < int(data.shape[0]):
        b1 = _cut(data, b0, chunk_bytes)
        chunks.append((b0, b1))
        b0 = b1
    return chunks


def host_record(raw: bytes, item_id_key: str):
    """One line by the host reader's own expressions: ``BLANK``, ``SKIPPED``
    or ``(user id, item id, rating, helpful_vote, verified, timestamp,
    ts_valid, text)`` with the strings encoded ``surrogatepass``. Raises what
    ``review_columns_from_jsonl`` raises on the line, and TypeError for an id
    that is not a string."""
    line = raw.decode("utf-8", "replace")
    if not line.strip():
        return BLANK
    r = json.loads(line)
    uid, iid, rt = r.get("user_id"), r.get(item_id_key), r.get("rating")
    if rt is None or not (uid and iid):
        return SKIPPED
    hash(uid), hash(iid)     # the reader's dicts refuse an unhashable id first
    rating = float(rt)
    helpful = _as_int(r.get("helpful_vote", 0)) or 0
    verified = bool(r.get("verified_purchase", False))
    t = _as_int(r.get("timestamp"))
    s = " ".join((r.get("title") or "", r.get("text") or ""))
    if not (isinstance(uid, str) and isinstance(iid, str)):
        raise TypeError("user_id and the item id must be strings")
    return (uid.encode("utf-8", "surrogatepass"), iid.encode("utf-8", "surrogatepass"), rating,
            helpful, verified, 0 if t is None else t, t is not None,
            s.encode("utf-8", "surrogatepass"))


class _Chunk(NamedTuple):
    """The compact outputs of one chunk (device tensors; offsets [records])."""
    rating: torch.Tensor
    helpful: torch.Tensor
    verified: torch.Tensor
    timestamp: torch.Tensor
    ts_valid: torch.Tensor
    user: tuple             # (data, offsets)
    item: tuple
    text: tuple
    counts: tuple           # lines, blank, skipped, records, flagged


class _Reader:
    """The launches of one chunk, one method each (tools/jsonl_bench.py times
    them one by one); ``run`` is their order."""

    def __init__(self, d: torch.Tensor, key: torch.Tensor, item_id_key: str, line_bytes):
        self.d, self.dev, self.key, self.item_id_key = d, d.device, key, item_id_key
        self.line_bytes = line_bytes       # (beg, end) -> the chunk's bytes on the host; None:
                                           # the source is on the device (one gather fetches them)
        self.deferred = None
        a = self.a = _lib.JsonlArgs()
        self.totals = torch.zeros(4, dtype=torch.int64, device=self.dev)
        a.n_bytes, a.data, a.totals = d.numel(), ptr(d), ptr(self.totals)
        a.item_key, a.item_key_len = ptr(key), key.numel()
        self.ref = ctypes.byref(a)
        self.side = None

    def count(self) -> None:
        call("bbgr_jsonl_count", self.ref, stream_handle())

    def read_lines(self) -> None:
        self.n_lines = self.a.n_lines = int(self.totals[0])

    def lines(self) -> None:
        n = self.n_lines
        self.line_end = torch.empty(max(n, 1), dtype=torch.int32, device=self.dev)
        self.a.line_end = ptr(self.line_end)
        _lib.call_with_workspace("bbgr_jsonl_lines", self.ref, device=self.dev)

    def scan(self) -> None:
        n, dev, a = max(self.n_lines, 1), self.dev, self.a
        self.status = torch.empty(n, dtype=torch.uint8, device=dev)
        self.rating = torch.empty(n, dtype=torch.float32, device=dev)
        self.helpful = torch.empty(n, dtype=torch.int32, device=dev)
        self.verified = torch.empty(n, dtype=torch.uint8, device=dev)
        self.timestamp = torch.empty(n, dtype=torch.int64, device=dev)
        self.ts_valid = torch.empty(n, dtype=torch.uint8, device=dev)
        self.sizes = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.spos = torch.empty((n, 4), dtype=torch.int32, device=dev)
        a.status, a.rating, a.helpful_vote = ptr(self.status), ptr(self.rating), ptr(self.helpful)
        a.verified, a.timestamp, a.ts_valid = (ptr(self.verified), ptr(self.timestamp),
                                               ptr(self.ts_valid))
        a.sizes, a.spos = ptr(self.sizes), ptr(self.spos)
        call("bbgr_jsonl_scan", self.ref, stream_handle())

    def read_scan(self) -> None:
        self.blank, self.skipped, self.kept, self.flagged = (int(v) for v in self.totals.tolist())

    def _flagged_bytes(self, begs: list, ends: list) -> list:
        """The bytes of the lines [beg, end): slices of the host source, or for
        a source on the device one gather and one copy for all of them."""
        if self.line_bytes is not None:
            return [self.line_bytes(b, e) for b, e in zip(begs, ends)]
        beg = torch.tensor(begs, dtype=torch.int64, device=self.dev)
        lens = torch.tensor(ends, dtype=torch.int64, device=self.dev) - beg
        at = torch.cumsum(lens, 0) - lens
        total = int(sum(ends) - sum(begs))
        pick = torch.repeat_interleave(beg - at, lens) + torch.arange(total, device=self.dev)
        raw, at = self.d[pick].cpu().numpy().tobytes(), at.tolist()
        return [raw[a:a + e - b] for a, b, e in zip(at, begs, ends)]

    def host_pass(self) -> None:
        """The flagged lines, in file order, by ``host_record``; what they
        give goes back into the per-line columns, their bytes into ``side``."""
        if not self.flagged:
            return
        idx = torch.nonzero(self.status[:self.n_lines] == FLAGGED).flatten()
        ends = self.line_end[idx].tolist()
        begs = [0 if l == 0 else e + 1 for l, e in
                zip(idx.tolist(), self.line_end[(idx - 1).clamp(min=0)].tolist())]
        status, rows, sizes, spos, side = [], [], [], [], bytearray()
        for raw in self._flagged_bytes(begs, ends):
            rec = host_record(raw, self.item_id_key)
            if rec in (BLANK, SKIPPED):
                status.append(rec)
                rows.append((0.0, 0, False, 0, False))
                sizes.append((0, 0, 0, 0))
                spos.append((-1, -1, -1, -1))
                self.blank += rec == BLANK
                self.skipped += rec == SKIPPED
                continue
            uid, iid, rating, helpful, verified, ts, ts_valid, text = rec
            status.append(HOST)
            rows.append((rating, helpful, verified, ts, ts_valid))
            at = len(side)
            sizes.append((len(uid), len(iid), len(text), 0))
            spos.append((at, at + len(uid), at + len(uid) + len(iid), -1))
            side += uid + iid + text
            self.kept += 1
        dev = self.dev

        def column(k, dtype):
            try:       # as the reader's np.asarray at its end: a value outside the type
                a = np.asarray([r[k] for r in rows], dtype)
            except OverflowError as e:
                self.deferred = self.deferred or e
                a = np.zeros(len(rows), dtype)
            return torch.from_numpy(a).to(dev)
        self.status[idx] = torch.tensor(status, dtype=torch.uint8, device=dev)
        self.rating[idx] = column(0, np.float32)
        self.helpful[idx] = column(1, np.int32)
        self.verified[idx] = column(2, np.uint8)
        self.timestamp[idx] = column(3, np.int64)
        self.ts_valid[idx] = column(4, np.uint8)
        self.sizes[idx] = torch.tensor(sizes, dtype=torch.int32, device=dev)
        self.spos[idx] = torch.tensor(spos, dtype=torch.int32, device=dev)
        if side:
            self.side = torch.from_numpy(np.frombuffer(side, np.uint8)).to(dev)
            self.a.side, self.a.side_bytes = ptr(self.side), self.side.numel()

    def offsets(self) -> None:
        self.offs = torch.empty((4, self.n_lines + 1), dtype=torch.int64, device=self.dev)
        self.a.offs = ptr(self.offs)
        _lib.call_with_workspace("bbgr_jsonl_offsets", self.ref, device=self.dev)

    def read_offsets(self) -> None:
        a = self.a
        a.n_records, a.user_bytes, a.item_bytes, a.text_bytes = (
            int(v) for v in self.offs[:, self.n_lines].tolist())

    def write(self) -> None:
        a, dev = self.a, self.dev
        n = int(a.n_records)

        def buf(size, dtype):
            return torch.empty(max(int(size), 1), dtype=dtype, device=dev)
        self.out = [buf(n, torch.float32), buf(n, torch.int32), buf(n, torch.uint8),
                    buf(n, torch.int64), buf(n, torch.uint8)]
        self.strs = [(buf(b, torch.uint8), buf(n, torch.int64))
                     for b in (a.user_bytes, a.item_bytes, a.text_bytes)]
        (a.out_rating, a.out_helpful, a.out_verified, a.out_timestamp,
         a.out_ts_valid) = (ptr(t) for t in self.out)
        (a.user_data, a.user_off), (a.item_data, a.item_off), (a.text_data, a.text_off) = (
            (ptr(x), ptr(o)) for x, o in self.strs)
        call("bbgr_jsonl_write", self.ref, stream_handle())

    def run(self) -> _Chunk:
        self.count()
        self.read_lines()
        if self.n_lines == 0:
            e = torch.empty(0, dtype=torch.uint8, device=self.dev)
            o = torch.empty(0, dtype=torch.int64, device=self.dev)
            return _Chunk(e.float(), e.int(), e, o, e, (e, o), (e, o), (e, o), (0, 0, 0, 0, 0))
        self.lines()
        self.scan()
        self.read_scan()
        self.host_pass()
        self.offsets()
        self.read_offsets()
        self.write()
        a, n = self.a, int(self.a.n_records)
        sizes = (a.user_bytes, a.item_bytes, a.text_bytes)
        strs = [(x[:b], o[:n]) for (x, o), b in zip(self.strs, sizes)]
        return _Chunk(*(t[:n] for t in self.out), *strs,
                      (self.n_lines, self.blank, self.skipped, n, self.flagged))


def _joined(parts: list, dev) -> tuple:
    """(data, offsets [n + 1]) of the chunks' (data, offsets [n]) pairs."""
    data = torch.cat([p[0] for p in parts]) if parts else torch.empty(0, dtype=torch.uint8, device=dev)
    offs, base = [], 0
    for x, o in parts:
        offs.append(o + base)
        base += x.numel()
    offs.append(torch.tensor([base], dtype=torch.int64, device=dev))
    return data, torch.cat(offs)


def _number_on_host(data: torch.Tensor, off: torch.Tensor, dev):
    raw, o = data.cpu().numpy().tobytes(), off.cpu().tolist()
    seen: dict = {}
    ids = np.fromiter((seen.setdefault(raw[o[r]:o[r + 1]], len(seen)) for r in range(len(o) - 1)),
                      np.int32, len(o) - 1)
    lens = np.zeros(len(seen) + 1, np.int64)
    if seen:
        np.cumsum([len(b) for b in seen], out=lens[1:])
    tab = np.frombuffer(bytearray().join(seen), np.uint8)
    return (torch.from_numpy(ids).to(dev),
            IdTable(torch.from_numpy(tab).to(dev), torch.from_numpy(lens).to(dev)))


def number_ids(data: torch.Tensor, off: torch.Tensor, hash_mask: int = 0):
    """``(ids int32 [n], IdTable, fallback)`` of the n id strings
    ``data[off[r]:off[r + 1]]`` (device tensors), numbered by first appearance:
    ``bbgr_ids_number`` and ``bbgr_ids_table``, or, when two different strings
    share a hash (``fallback``), a dict on the host over the same bytes."""
    dev, n = data.device, off.numel() - 1
    if n >= BYTES_MAX:
        raise ValueError(f"n = {n} records: n must be < 2^31 - 1")
    if n == 0:
        z = torch.zeros(1, dtype=torch.int64, device=dev)
        return (torch.empty(0, dtype=torch.int32, device=dev),
                IdTable(torch.empty(0, dtype=torch.uint8, device=dev), z), False)
    d = data if data.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    first_rec = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.call_with_workspace("bbgr_ids_number", n, ptr(d), ptr(off), data.numel(), int(hash_mask),
                             ptr(ids), ptr(first_rec), ptr(totals), device=dev)
    n_ids, collisions = (int(v) for v in totals.tolist())
    if collisions:
        return (*_number_on_host(data, off, dev), True)
    tab_off = torch.empty(n_ids + 1, dtype=torch.int64, device=dev)
    args = (n_ids, ptr(first_rec), n, ptr(d), ptr(off), data.numel(), ptr(tab_off))
    _lib.call_with_workspace("bbgr_ids_table", *args, None, 0, device=dev)
    tab_bytes = int(tab_off[-1])
    tab = torch.empty(max(tab_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.call_with_workspace("bbgr_ids_table", *args, ptr(tab), tab_bytes, device=dev)
    return ids, IdTable(tab[:tab_bytes], tab_off), False


def read_reviews(src, item_id_key: str = "parent_asin", device="cuda",
                 chunk_bytes: int = 1 << 30, _hash_mask: int = 0) -> ParsedReviews:
    """The records of a review dump (module docstring). ``src``: a path
    (memory-mapped, never read whole), ``bytes`` / ``bytearray``, a uint8
    numpy array or a uint8 tensor (one on the GPU is used where it is).
    ValueError, before any launch, for an ``item_id_key`` that is not ASCII
    without quote, backslash and control bytes (or longer than 255 bytes),
    and, before that chunk's launch, for a line of ``BYTES_MAX`` bytes or
    more. ``_hash_mask`` narrows the numbering's hash (tests: it forces the
    host numbering, reported in ``info["numbering_fallback"]``)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("read_reviews runs on the GPU; there is no CPU fallback")
    key = _key_bytes(item_id_key)
    chunk_bytes = _chunk_bytes(chunk_bytes)
    data = _source(src)
    _lib.require_gpu()
    with torch.cuda.device(data.device if isinstance(data, torch.Tensor) else device):
        dev = torch.device("cuda", torch.cuda.current_device())
        key_dev = torch.from_numpy(np.frombuffer(key, np.uint8).copy()).to(dev)
        parts, deferred, n_chunks, b0, n = [], None, 0, 0, int(data.shape[0])
        while b0 < n:       # planned chunk by chunk: a long line raises before its own launch
            b1 = _cut(data, b0, chunk_bytes)
            piece = data[b0:b1]
            if isinstance(piece, torch.Tensor):
                d = piece
            else:
                d = torch.from_numpy(np.array(piece)).to(dev)      # one host copy: a map is read-only
            rd = _Reader(d, key_dev, item_id_key, None if isinstance(piece, torch.Tensor) else
                         (lambda beg, end, piece=piece: np.asarray(piece[beg:end]).tobytes()))
            parts.append(rd.run())
            deferred = deferred or rd.deferred
            n_chunks += 1
            b0 = b1
        if deferred is not None:
            raise deferred
        counts = np.asarray([p.counts for p in parts], np.int64).reshape(-1, 5).sum(0)

        def cat(name, dtype):
            ts = [getattr(p, name) for p in parts]
            return torch.cat(ts) if ts else torch.empty(0, dtype=dtype, device=dev)
        users = _joined([p.user for p in parts], dev)
        items = _joined([p.item for p in parts], dev)
        text = ReviewText(*_joined([p.text for p in parts], dev))
        user, user_ids, fb_u = number_ids(*users, _hash_mask)
        item, item_ids, fb_i = number_ids(*items, _hash_mask)
        n_tok, n_uniq, _ = token_counts(text, dev)
        cols = ReviewColumns(
            user=user, item=item, rating=cat("rating", torch.float32),
            helpful_vote=cat("helpful", torch.int32), verified=cat("verified", torch.uint8),
            timestamp=cat("timestamp", torch.int64), n_tokens=n_tok, n_unique_tokens=n_uniq,
            ts_valid=cat("ts_valid", torch.uint8).bool(), text=text)
        info = {"lines": int(counts[0]), "records": int(counts[3]), "blank": int(counts[1]),
                "skipped": int(counts[2]), "flagged": int(counts[4]),
                "numbering_fallback": int(fb_u) + int(fb_i),
                "chunks": n_chunks}
        return ParsedReviews(cols, user_ids, item_ids, info)
