"""Review text -> token and distinct-token counts, on the device.

Restates, over the UTF-8 bytes of each record's ``title + " " + text``::

    toks = re.findall(r"[a-z]+(?:'[a-z]+)?", s.lower())     # main.py tokenize()
    n_tokens, n_unique_tokens = len(toks), len(set(toks))

the two integers per record that ``build_credibility_graph`` turns into
``lexical_diversity`` and ``review_length_discrepancy``::

    text = ReviewText.from_strings(strings)
    n_tokens, n_unique_tokens, info = token_counts(text)

The rule over bytes: a letter is an ASCII ``A-Za-z`` compared as
its lower case, or the byte ``C4`` of U+0130 (``İ``, whose ``lower()`` is ``i``
+ U+0307); ``'`` is the apostrophe; every other byte and a record's edge
separate. With this Python's Unicode tables, U+0130 and U+212A (Kelvin sign,
``lower()`` = ``k``) are the only code points outside ASCII whose ``lower()``
holds a character of ``[a-z']`` (tests/test_text_host.py enumerates them).
The Kelvin sign is the one letter that is not one byte: the device flags every
record that holds it, and so every record in which two different tokens share
a hash (none with the full 64 bits on any text seen so far; the comparison of
the tokens' bytes on the device is what makes an unflagged record exact, not
merely probable). Flagged records are counted again here on the host with
``features.tokenize``.

``pooled_token_counts`` counts over all records of a group (the user) instead:
``|set of all the group's tokens|`` and the group's token total, what
main_v2_.py's pooled ``lexical_diversity`` divides. Equal tokens of different
records must meet, but only inside a group. By default the text is ONE chunk
(below 2^31 - 1 bytes). With ``chunk_bytes`` it may be of any size: the records
are grouped on the device (``bbgr_csr_build``), the group ids cut into
consecutive ranges whose records fit a chunk (``plan_group_ranges``), each
range's records packed back to back (``bbgr_text_gather``) and counted by the
one-chunk kernel with group ids local to the range. Every count and flag of
``bbgr_text_unique_pooled`` depends on the multiset of a group's tokens, not on
the order of its records, so the result is bit for bit the one-chunk one; no
device-resident vocabulary is needed. Flagged groups (one that owns a Kelvin
record, or in which two different tokens share a hash) are counted again here
on the host over the group's records.

Launches per chunk: ``bbgr_text_count`` (one host read of the token total,
which sizes the workspace), ``bbgr_text_unique``, one host read of the number
of flagged records. Integer work only: two calls give the same bits.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_handle
from .features import tokenize

BYTES_MAX = 2**31 - 1     # a chunk's bytes and a call's records stay below this
TEXT_STEP = 64            # bytes a wave reads per step (csrc/text.hip)


class ReviewText(NamedTuple):
    """The text of the records, in file order: ``data`` the UTF-8 bytes of
    every record back to back (uint8), ``offsets`` int64 [n + 1] with record r
    at ``data[offsets[r]:offsets[r + 1]]`` (numpy arrays or tensors; bytes
    already on the GPU are used where they are)."""
    data: object
    offsets: object

    def __len__(self) -> int:
        return int(self.offsets.shape[0]) - 1

    @classmethod
    def from_strings(cls, strings) -> "ReviewText":
        """``surrogatepass``: ``json.loads`` can return a lone surrogate, which a
        plain encode refuses; its three bytes are separators like any others
        of 0x80 and above."""
        return cls.from_encoded([s.encode("utf-8", "surrogatepass") for s in strings])

    @classmethod
    def from_encoded(cls, enc: list) -> "ReviewText":
        offsets = np.zeros(len(enc) + 1, np.int64)
        if enc:
            np.cumsum([len(b) for b in enc], out=offsets[1:])
        return cls(np.frombuffer(bytearray().join(enc), np.uint8), offsets)   # writable: no copy later


def _checked_text(text: ReviewText):
    """(data, offsets): the offsets as host int64 after the checks; the bytes
    as they came, a host array or, for a tensor on a GPU, that tensor (it is
    not brought back to the host)."""
    data = text.data
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("text.data must be a uint8 vector")
        data = data.contiguous() if data.is_cuda else data.numpy()
    else:
        data = np.asarray(data)
    if not isinstance(data, torch.Tensor):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("text.data must be a uint8 vector")
        data = np.ascontiguousarray(data)
    off = (text.offsets.cpu().numpy() if isinstance(text.offsets, torch.Tensor)
           else np.asarray(text.offsets))
    if off.ndim != 1 or off.shape[0] < 1 or off.dtype != np.int64:
        raise ValueError("text.offsets must be an int64 vector of n + 1 entries")
    if off[0] < 0 or off[-1] > data.shape[0]:
        raise ValueError(f"text.offsets span [{int(off[0])}, {int(off[-1])}], outside the "
                         f"{data.shape[0]} bytes of data")
    if off.shape[0] > 1 and bool((np.diff(off) < 0).any()):
        raise ValueError("text.offsets must not decrease")
    return data, np.ascontiguousarray(off)


def _bytes_to(a, dev) -> torch.Tensor:
    """A non-empty byte range on the device: one copy for a host array (a
    read-only one, such as a memory map, is copied on the host first: torch
    wants a writable one), none for a tensor that is there already."""
    if isinstance(a, torch.Tensor):
        return a.to(dev)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def _record_bytes(data, b0: int, b1: int) -> bytes:
    a = data[b0:b1]
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _plan_ranges(prefix: np.ndarray, chunk_bytes: int, what: str) -> list:
    """[(i0, i1), ..]: consecutive index ranges that cover [0, len(prefix) - 1),
    each of at most ``chunk_bytes`` bytes by the prefix sums, taking as many
    entries as fit; an entry larger than that is a range of its own."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be at least 1")
    chunk_bytes = min(chunk_bytes, BYTES_MAX - 1)
    n = int(prefix.shape[0]) - 1
    if n and int(np.diff(prefix).max()) >= BYTES_MAX:
        r = int(np.diff(prefix).argmax())
        raise ValueError(f"{what} {r} has {int(prefix[r + 1] - prefix[r])} bytes: a {what} "
                         "must be shorter than 2^31 - 1 bytes")
    ranges, r0 = [], 0
    while r0 < n:
        # the last r1 with prefix[r1] - prefix[r0] <= chunk_bytes
        r1 = int(np.searchsorted(prefix, prefix[r0] + chunk_bytes, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        ranges.append((r0, r1))
        r0 = r1
    return ranges


def plan_chunks(offsets: np.ndarray, chunk_bytes: int) -> list:
    """[(r0, r1), ..]: consecutive record ranges that cover every record, each
    of at most ``chunk_bytes`` bytes, taking as many records as fit; a record
    longer than that is a range of its own. ValueError for a record of
    2^31 - 1 bytes or more."""
    return _plan_ranges(offsets, chunk_bytes, "record")


def plan_group_ranges(group_bytes_prefix: np.ndarray, chunk_bytes: int) -> list:
    """[(g0, g1), ..]: consecutive group-id ranges that cover ``[0, G)``, from
    the int64 [G + 1] prefix sums of the groups' bytes: ``plan_chunks``' rule
    over groups. Each range takes as many groups as fit in ``chunk_bytes``
    (capped at 2^31 - 2); a group larger than that is a range of its own.
    ValueError for ``chunk_bytes < 1`` and, naming the group and its size, for
    a group of 2^31 - 1 bytes or more."""
    return _plan_ranges(np.asarray(group_bytes_prefix), chunk_bytes, "group")


def _text_args(data: torch.Tensor, off: torch.Tensor, first: int, last: int, hash_mask: int,
               n_tok: torch.Tensor, n_uniq: torch.Tensor, recheck: torch.Tensor,
               totals: torch.Tensor) -> _lib.TextArgs:
    a = _lib.TextArgs()
    a.n, a.data, a.offsets = n_tok.numel(), ptr(data), ptr(off)
    a.first, a.last, a.hash_mask = first, last, hash_mask
    a.n_tokens, a.n_unique_tokens = ptr(n_tok), ptr(n_uniq)
    a.recheck, a.totals = ptr(recheck), ptr(totals)
    return a


def _run_chunk(data: torch.Tensor, off: torch.Tensor, first: int, last: int, hash_mask: int,
               n_tok: torch.Tensor, n_uniq: torch.Tensor, recheck: torch.Tensor,
               totals: torch.Tensor) -> tuple:
    """Both calls on device tensors: ``data`` the chunk's bytes (record r at
    ``data[off[r]:off[r + 1]]``, ``first`` / ``last`` the host copies of
    ``off[0]`` / ``off[-1]``), outputs [n]. Returns (tokens, flagged)."""
    a = _text_args(data, off, first, last, hash_mask, n_tok, n_uniq, recheck, totals)
    st = stream_handle()
    call("bbgr_text_count", ctypes.byref(a), st)
    tokens = int(totals[0])                                  # the host read that sizes the workspace
    _lib.call_with_workspace("bbgr_text_unique", ctypes.byref(a), tokens, after=(st,),
                             device=data.device)
    return tokens, int(totals[1])


def host_counts(record: bytes) -> tuple:
    """(n_tokens, n_unique_tokens) of one record's bytes by ``features.tokenize``."""
    toks = tokenize(record.decode("utf-8", "surrogatepass"))
    return len(toks), len(set(toks))


def token_counts(text: ReviewText, device="cuda", chunk_bytes: int = 1 << 30, _hash_mask: int = 0):
    """``(n_tokens, n_unique_tokens, info)``: int32 [n] device tensors and
    ``info = {"tokens", "rechecked", "chunks"}`` (the token total, the records
    counted again on the host, the chunks run). The records go to the device
    in chunks of at most ``chunk_bytes`` bytes (and below 2^31 - 1); a longer
    record is a chunk of its own, and one of 2^31 - 1 bytes or more a
    ValueError before any launch. ``_hash_mask`` narrows the hash (tests: it
    forces collisions, which only raise ``rechecked``)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("token_counts runs on the GPU; there is no CPU fallback")
    data, off = _checked_text(text)
    n = off.shape[0] - 1
    if n >= BYTES_MAX:
        raise ValueError(f"n = {n} records: n must be < 2^31 - 1")
    chunks = plan_chunks(off, chunk_bytes)
    _lib.require_gpu()
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        n_tok = torch.zeros(n, dtype=torch.int32, device=dev)
        n_uniq = torch.zeros(n, dtype=torch.int32, device=dev)
        recheck = torch.zeros(n, dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        flagged = 0
        for r0, r1 in chunks:
            b0, b1 = int(off[r0]), int(off[r1])
            # the kernels read [0, b1 - b0) only; an empty chunk still needs an address
            d = (_bytes_to(data[b0:b1], dev) if b1 > b0
                 else torch.zeros(1, dtype=torch.uint8, device=dev))
            o = torch.from_numpy(off[r0:r1 + 1] - b0).to(dev)
            flagged += _run_chunk(d, o, 0, b1 - b0, int(_hash_mask), n_tok[r0:r1], n_uniq[r0:r1],
                                  recheck[r0:r1], totals)[1]
        if flagged:
            idx = torch.nonzero(recheck).flatten()
            fixed = np.empty((idx.numel(), 2), np.int32)
            for k, r in enumerate(idx.tolist()):
                fixed[k] = host_counts(_record_bytes(data, int(off[r]), int(off[r + 1])))
            fixed_dev = torch.from_numpy(fixed).to(dev)
            n_tok[idx] = fixed_dev[:, 0]
            n_uniq[idx] = fixed_dev[:, 1]
        info = {"tokens": int(n_tok.sum(dtype=torch.int64)), "rechecked": flagged,
                "chunks": len(chunks)}
        return n_tok, n_uniq, info


def _check_groups(group, n: int, num_groups: int) -> None:
    shape = tuple(group.shape)
    if len(shape) != 1 or shape[0] != n:
        raise ValueError(f"group: expected {n} entries, got shape {shape}")
    if n == 0:
        return
    if isinstance(group, torch.Tensor):
        lo, hi = (int(v) for v in torch.aminmax(group))
    else:
        lo, hi = int(np.min(group)), int(np.max(group))
    if lo < 0 or hi >= num_groups:
        raise ValueError(f"group id out of range: [{lo}, {hi}] not within "
                         f"[0, num_groups = {num_groups})")


UPLOAD_PIECE = 1 << 30    # bytes of a host array that go to the device in one copy


def _upload(data: np.ndarray, dev) -> torch.Tensor:
    """A host byte array as one device tensor, copied in pieces of at most
    ``UPLOAD_PIECE`` bytes: no second whole copy on the host (torch wants a
    writable source, so a read-only piece is copied first)."""
    n = int(data.shape[0])
    d = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    for a in range(0, n, UPLOAD_PIECE):
        piece = data[a:a + UPLOAD_PIECE]
        d[a:a + piece.shape[0]].copy_(torch.from_numpy(piece if piece.flags.writeable
                                                       else piece.copy()))
    return d


def resident(text: ReviewText, device="cuda") -> ReviewText:
    """``text`` with its bytes in one device tensor (uploaded once, in pieces;
    a tensor on a GPU is used where it is) and its offsets as they came: what
    ``token_counts`` and ``pooled_token_counts(.., chunk_bytes=..)`` both read
    without another copy of the bytes."""
    data, _ = _checked_text(text)
    if isinstance(data, torch.Tensor):
        return ReviewText(data, text.offsets)
    _lib.require_gpu()
    with torch.cuda.device(torch.device(device)):
        dev = torch.device("cuda", torch.cuda.current_device())
        return ReviewText(_upload(data, dev), text.offsets)


def _recount_flagged(data, off: np.ndarray, grp: torch.Tensor, G: int, g_flag: torch.Tensor,
                     g_tok: torch.Tensor, g_uniq: torch.Tensor) -> None:
    """The flagged groups counted again on the host over their records."""
    idx = torch.nonzero(g_flag).flatten()
    g_host = grp.cpu().numpy()
    order = np.argsort(g_host, kind="stable")
    starts = np.searchsorted(g_host[order], np.arange(G + 1))
    fixed = np.empty((idx.numel(), 2), np.int64)
    for k, g in enumerate(idx.tolist()):
        seen, total = set(), 0
        for r in order[starts[g]:starts[g + 1]].tolist():
            toks = tokenize(_record_bytes(data, int(off[r]), int(off[r + 1]))
                            .decode("utf-8", "surrogatepass"))
            total += len(toks)
            seen.update(toks)
        fixed[k] = (total, len(seen))
    fixed_dev = torch.from_numpy(fixed).to(grp.device)
    g_tok[idx] = fixed_dev[:, 0]
    g_uniq[idx] = fixed_dev[:, 1].to(torch.int32)


def _pooled_chunked(data, off: np.ndarray, grp: torch.Tensor, G: int, hash_mask: int,
                    g_tok: torch.Tensor, g_uniq: torch.Tensor, g_flag: torch.Tensor,
                    chunk_bytes: int, group_csr) -> tuple:
    """The regrouped count (module docstring) into g_tok / g_uniq / g_flag:
    (flagged groups, Kelvin records, ranges of the plan). Host reads: the
    groups' byte totals and row bounds once for the plan; per range the token
    total, which sizes the workspace."""
    dev = grp.device
    n = off.shape[0] - 1
    # a host array goes up from its first record's byte to its last's only; a tensor stays whole
    base = 0 if isinstance(data, torch.Tensor) else int(off[0])
    d = data if isinstance(data, torch.Tensor) else _upload(data[base:int(off[-1])], dev)
    o = torch.from_numpy(off - base).to(dev)
    if group_csr is None:
        from .features import _group
        group_csr = _group(grp, torch.zeros(max(n, 1), dtype=torch.int32, device=dev), G)
    indptr, eid = group_csr
    if indptr.dtype != torch.int32 or eid.dtype != torch.int32 or indptr.numel() != G + 1 \
            or eid.numel() < n or not (indptr.is_cuda and eid.is_cuda):
        raise ValueError("group_csr: (indptr int32 [G + 1], record ids int32 [n]) device tensors")
    # the groups' bytes: the running sum of the record lengths in group order, at the row bounds
    run = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum((o[1:] - o[:-1])[eid[:n].long()], 0, out=run[1:])
    prefix = run[indptr.long()].cpu().numpy()
    rows = indptr.cpu().numpy().astype(np.int64)
    del run
    plan = plan_group_ranges(prefix, chunk_bytes)
    ranges = [(g0, g1) for g0, g1 in plan if rows[g1] > rows[g0]]   # the others launch nothing
    g_tok.zero_()       # a group in a range without a record gets 0 / 0
    g_uniq.zero_()
    g_flag.zero_()
    flagged = torch.zeros((), dtype=torch.int64, device=dev)
    kelvin = torch.zeros((), dtype=torch.int64, device=dev)
    if not ranges:
        return 0, 0, len(plan)
    # one buffer of the largest range's bytes and records, sized from the plan: no host read
    cap = max(int(prefix[g1] - prefix[g0]) for g0, g1 in ranges)
    m_max = max(int(rows[g1] - rows[g0]) for g0, g1 in ranges)
    chunk = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    c_off = torch.empty(m_max + 1, dtype=torch.int64, device=dev)
    n_tok = torch.empty(m_max, dtype=torch.int32, device=dev)
    n_uniq = torch.empty(m_max, dtype=torch.int32, device=dev)     # bbgr_text_args wants one
    recheck = torch.empty(m_max, dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    c_total = torch.empty(1, dtype=torch.int64, device=dev)
    ws_gather, ws_pooled = _lib.Workspace(), _lib.Workspace()
    ga = _lib.TextGatherArgs()
    ga.n, ga.data, ga.offsets = n, ptr(d), ptr(o)
    ga.first, ga.last = int(off[0]) - base, int(off[-1]) - base
    ga.out_offsets, ga.out_data, ga.total = ptr(c_off), ptr(chunk), ptr(c_total)
    st = stream_handle()
    for g0, g1 in ranges:
        e0, e1 = int(rows[g0]), int(rows[g1])
        m, nbytes = e1 - e0, int(prefix[g1] - prefix[g0])
        recs = eid[e0:e1]
        ga.n_list, ga.records, ga.capacity = m, ptr(recs), nbytes
        _lib.call_with_workspace("bbgr_text_gather", ctypes.byref(ga), after=(st,), device=dev,
                                 keep=ws_gather)
        local = (grp[recs.long()] - g0).contiguous()
        a = _text_args(chunk, c_off, 0, nbytes, hash_mask, n_tok[:m], n_uniq[:m], recheck[:m],
                       totals)
        call("bbgr_text_count", ctypes.byref(a), st)
        tokens = int(totals[0])                                  # sizes the workspace
        _lib.call_with_workspace("bbgr_text_unique_pooled", ctypes.byref(a), tokens, ptr(local),
                                 g1 - g0, ptr(g_tok[g0:g1]), ptr(g_uniq[g0:g1]),
                                 ptr(g_flag[g0:g1]), after=(st,), device=dev, keep=ws_pooled)
        flagged += totals[1]
        kelvin += recheck[:m].sum(dtype=torch.int64)
    return int(flagged), int(kelvin), len(plan)


def pooled_token_counts(text: ReviewText, group, num_groups: int, device="cuda",
                        _hash_mask: int = 0, out=None, chunk_bytes=None, group_csr=None):
    """``(tokens, unique, info)`` per group: int64 [G] the sum of the token
    counts of the group's records, int32 [G] the distinct tokens over all of
    them (device tensors; a group without a record gets 0 and 0), and ``info =
    {"tokens", "rechecked", "kelvin_records"}``: the token total, the groups
    counted again on the host, the records that hold U+212A. ``group``: int32
    [n], the group of each record (a host array or a tensor, also one on the
    device). ``out``: optional ``(tokens, unique)`` device tensors to write.
    ValueError before any launch for a group outside ``[0, num_groups)`` and,
    with ``chunk_bytes=None``, for text of 2^31 - 1 bytes or more: the text is
    one chunk (module docstring). ``_hash_mask`` as for ``token_counts``.

    ``chunk_bytes=<int>``: text of any size, regrouped by group into chunks of
    at most that many bytes (module docstring); a group larger than that runs
    alone, and one of 2^31 - 1 bytes or more is a ValueError. The text goes to
    the device once (a device tensor is used where it is; a host array is
    uploaded in pieces of at most 1 GiB), and the same counts and ``info``
    come back, with ``info["chunks"]`` the number of ranges of the plan
    (``len(plan_group_ranges(..))``). A range whose groups have no record
    launches nothing and is counted all the same, so ``"chunks"`` can exceed
    the ranges actually run by the number of such ranges (trailing or leading
    groups without a record that do not fit their neighbour's range).
    Device memory: the text, one chunk and that chunk's workspace (40 bytes
    per token); beside them the offsets (8 bytes per record, for the whole
    call), while the plan is made about 32 bytes per record of int64
    temporaries (lengths, record ids, their running sum; freed before the
    first range) and 8 bytes per group, and per range 20 bytes per record of
    the range (its packed offsets, ids and local groups, the count columns).
    ``group_csr``: optional ``(indptr int32 [G + 1], record ids int32 [n])``
    device tensors, the records grouped by group (``bbgr_csr_build`` with the
    record id as the column) for a caller that holds them already."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("pooled_token_counts runs on the GPU; there is no CPU fallback")
    G = int(num_groups)
    if G < 0 or G >= BYTES_MAX:
        raise ValueError(f"num_groups = {G}: must lie in [0, 2^31 - 1)")
    if chunk_bytes is not None and int(chunk_bytes) < 1:
        raise ValueError("chunk_bytes must be at least 1")
    ends = (text.offsets.cpu().numpy() if isinstance(text.offsets, torch.Tensor)
            else np.asarray(text.offsets))
    if chunk_bytes is None and ends.ndim == 1 and ends.shape[0] > 1 \
            and int(ends[-1]) - int(ends[0]) >= BYTES_MAX:
        raise ValueError(f"text of {int(ends[-1]) - int(ends[0])} bytes: pooled counts take the "
                         "text as one chunk, which must be shorter than 2^31 - 1 bytes")
    data, off = _checked_text(text)
    n = off.shape[0] - 1
    if n >= BYTES_MAX:
        raise ValueError(f"n = {n} records: n must be < 2^31 - 1")
    if not isinstance(group, torch.Tensor):
        group = np.asarray(group)
    _check_groups(group, n, G)
    _lib.require_gpu()
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        grp = (group if isinstance(group, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(group))).to(device=dev, dtype=torch.int32).contiguous()
        if out is None:
            out = (torch.empty(G, dtype=torch.int64, device=dev),
                   torch.empty(G, dtype=torch.int32, device=dev))
        g_tok, g_uniq = out
        if (g_tok.dtype, g_uniq.dtype) != (torch.int64, torch.int32) or \
                not (g_tok.is_cuda and g_uniq.is_cuda and g_tok.is_contiguous()
                     and g_uniq.is_contiguous()) or g_tok.numel() != G or g_uniq.numel() != G:
            raise ValueError("out: (int64 [G], int32 [G]) contiguous device tensors")
        g_flag = torch.empty(G, dtype=torch.uint8, device=dev)
        if chunk_bytes is not None:
            flagged, kelvin, chunks = _pooled_chunked(
                data, off, grp, G, int(_hash_mask), g_tok, g_uniq, g_flag, int(chunk_bytes),
                group_csr)
            if flagged:
                _recount_flagged(data, off, grp, G, g_flag, g_tok, g_uniq)
            info = {"tokens": int(g_tok.sum()), "rechecked": flagged, "kelvin_records": kelvin,
                    "chunks": chunks}
            return g_tok, g_uniq, info
        b0, b1 = int(off[0]), int(off[-1])
        d = (_bytes_to(data[b0:b1], dev) if b1 > b0
             else torch.zeros(1, dtype=torch.uint8, device=dev))
        o = torch.from_numpy(off - b0).to(dev)
        n_tok = torch.zeros(n, dtype=torch.int32, device=dev)
        n_uniq = torch.zeros(n, dtype=torch.int32, device=dev)     # bbgr_text_args wants one
        recheck = torch.zeros(n, dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        a = _text_args(d, o, 0, b1 - b0, int(_hash_mask), n_tok, n_uniq, recheck, totals)
        st = stream_handle()
        call("bbgr_text_count", ctypes.byref(a), st)
        tokens = int(totals[0])                                  # sizes the workspace
        _lib.call_with_workspace("bbgr_text_unique_pooled", ctypes.byref(a), tokens, ptr(grp), G,
                                 ptr(g_tok), ptr(g_uniq), ptr(g_flag), after=(st,), device=dev)
        flagged = int(totals[1])
        if flagged:
            _recount_flagged(data, off, grp, G, g_flag, g_tok, g_uniq)
        info = {"tokens": int(g_tok.sum()), "rechecked": flagged,
                "kelvin_records": int(recheck.sum(dtype=torch.int64))}
        return g_tok, g_uniq, info
