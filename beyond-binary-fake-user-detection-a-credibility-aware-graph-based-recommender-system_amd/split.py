"""Review columns -> train / val / test edges, on the device.

Restates ``build_graph_from_jsonl`` (Version-2/lighgcn_cu_pop.py:227-303; the
same code opens every training script of the reference): keep the reviews with
``rating >= 4``, number users and items by first appearance among them, and
send every kept pair to train, val or test by ``split_bucket``: the first 8 hex
digits of md5 over ``"{uid}|{iid}"`` divided by 0xFFFFFFFF against 0.8 and
0.9. It joins the review reader to the recommender::

    cols, user2idx, item2idx = review_columns_from_jsonl("reviews.jsonl")
    split = split_interactions(cols.user, cols.item, cols.rating,
                               id_table(user2idx), id_table(item2idx))
    M_ui, M_iu = build_message_passing_mats(split.train.cpu().numpy(), split.num_users,
                                            split.num_items, split.cred(cred_all), "cuda")

The strings are one host pass (``id_table``); the hash, the numbering and the
partition run on the device (``bbgr_md5_pair_hash``, ``bbgr_split_edges``).
The two bucket boundaries are found once on the host with Python's own double
division (``split_thresholds``) and the device compares integers, so a record
lands where the reference's ``int(h[:8], 16) / 0xFFFFFFFF < p`` sends it for
every one of the 2^32 hash values. Everything is integer: two calls give the
same bits.

A record is what the reader keeps (``review_columns_from_jsonl`` drops an
empty-string id; the reference keeps it), and the positive test runs on the
float32 rating column.
"""
from __future__ import annotations

import ctypes
import pickle
from pathlib import Path
from typing import Iterable, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_handle

HASH_DENOM = 0xFFFFFFFF     # split_bucket divides by this, not by 2^32
N_MAX = 2**31 - 1


class IdTable(NamedTuple):
    """The id strings of one side, in id order: ``data`` the UTF-8 bytes of
    every id back to back (uint8), ``offsets`` int64 [n_ids + 1] with id k at
    ``data[offsets[k]:offsets[k + 1]]`` (numpy arrays or tensors)."""
    data: object
    offsets: object

    def __len__(self) -> int:
        return int(self.offsets.shape[0]) - 1


def id_table(ids: Iterable[str]) -> IdTable:
    """The table of an iterable of ``str`` in its order: of a dict
    ``{id: index}`` filled in first-appearance order (``user2idx`` of
    ``review_columns_from_jsonl``), the table of that index."""
    enc = [s.encode("utf-8") for s in ids]
    offsets = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum([len(b) for b in enc], out=offsets[1:])
    return IdTable(np.frombuffer(b"".join(enc), np.uint8), offsets)


def _smallest_not_below(p: float) -> int:
    """The smallest integer v in [0, 2^32] with not (v / 0xFFFFFFFF < p), in
    Python's double division: v / 0xFFFFFFFF is non-decreasing in v, so a
    bisection finds the boundary; 2^32 when every 32-bit value is below."""
    lo, hi = 0, 2**32          # the answer lies in [lo, hi]
    while lo < hi:
        mid = (lo + hi) // 2
        if mid / HASH_DENOM < p:
            lo = mid + 1
        else:
            hi = mid
    return lo


def split_thresholds(train_p: float = 0.8, val_p: float = 0.1) -> tuple[int, int]:
    """(thr_train, thr_val): hash32 < thr_train is train, hash32 < thr_val is
    val, the rest test, exactly where ``split_bucket`` draws the lines
    (``x < train_p``, ``x < train_p + val_p`` with the sum formed in double)."""
    train_p, val_p = float(train_p), float(val_p)
    total = train_p + val_p
    for name, v in (("train_p", train_p), ("val_p", val_p), ("train_p + val_p", total)):
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"{name} = {v} must lie in [0, 1]")
    return _smallest_not_below(train_p), _smallest_not_below(total)


class InteractionSplit(NamedTuple):
    """Device tensors of ``split_interactions``; ``counts`` is a host dict."""
    train: torch.Tensor       # int32 [2, E_train]: new user ids, new item ids
    val: torch.Tensor         # int32 [2, E_val]
    test: torch.Tensor        # int32 [2, E_test]
    user_src: torch.Tensor    # int32 [U']: the old id of a new user id
    item_src: torch.Tensor    # int32 [I']
    num_users: int            # U'
    num_items: int            # I'
    counts: dict              # train, val, test

    def cred(self, cred_all) -> torch.Tensor:
        """``cred_all[user_src]``: a per-user vector in the review reader's
        numbering (``bbgr.cred_train``'s ``cred_u``) in the recommender's."""
        c = cred_all if isinstance(cred_all, torch.Tensor) else torch.as_tensor(np.asarray(cred_all))
        return c.to(self.user_src.device)[self.user_src.long()]


def _device(device, who: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who} runs on the GPU; there is no CPU fallback")
    return device


def _host_table(t: IdTable, name: str):
    """(data uint8, offsets int64) as numpy after the host checks."""
    data = t.data.cpu().numpy() if isinstance(t.data, torch.Tensor) else np.asarray(t.data)
    off = t.offsets.cpu().numpy() if isinstance(t.offsets, torch.Tensor) else np.asarray(t.offsets)
    if data.dtype != np.uint8 or data.ndim != 1:
        raise ValueError(f"{name}.data must be a uint8 vector")
    if off.ndim != 1 or off.shape[0] < 1 or off.dtype != np.int64:
        raise ValueError(f"{name}.offsets must be an int64 vector of n_ids + 1 entries")
    if off[0] != 0:
        raise ValueError(f"{name}.offsets must start at 0, got {int(off[0])}")
    if off.shape[0] > 1 and bool((np.diff(off) < 0).any()):
        raise ValueError(f"{name}.offsets must not decrease")
    if off[-1] > data.shape[0]:
        raise ValueError(f"{name}.offsets end at {int(off[-1])}, past the {data.shape[0]} bytes "
                         "of data")
    if off.shape[0] - 1 >= N_MAX:
        raise ValueError(f"{name}: the id count must be < 2^31 - 1")
    return np.ascontiguousarray(data), np.ascontiguousarray(off)


def _length(x) -> int:
    if getattr(x, "ndim", 1) != 1:
        raise ValueError(f"columns are vectors, got shape {tuple(x.shape)}")
    return int(x.shape[0])


def _check_columns(user, item, n_users: int, n_items: int, **others) -> int:
    n = _length(user)
    for name, x in (("item", item), *others.items()):
        if x is not None and _length(x) != n:
            raise ValueError(f"column {name}: expected {n} entries, got {_length(x)}")
    if n >= N_MAX:
        raise ValueError(f"n = {n} records: n must be < 2^31 - 1")
    if n:
        for name, x, bound in (("user", user, n_users), ("item", item, n_items)):
            lo, hi = (int(v) for v in (torch.aminmax(x) if isinstance(x, torch.Tensor)
                                       else (np.min(x), np.max(x))))
            if lo < 0 or hi >= bound:
                raise ValueError(f"{name} id out of range: [{lo}, {hi}] not within "
                                 f"[0, {bound}), the {name} id table's size")
    return n


def _dev(x, dev, dtype) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(device=dev, dtype=dtype).contiguous()


def _threshold_f32(threshold: float) -> float:
    """The smallest float32 t with t >= threshold: for a float32 rating r,
    ``r >= t`` is ``float(r) >= threshold`` exactly, whatever the threshold."""
    t = np.float32(threshold)
    if float(t) < float(threshold):
        t = np.nextafter(t, np.float32(np.inf))
    return float(t)


def _hash_raw(hash32, dev) -> torch.Tensor:
    """A caller's hash column as the int32 bit patterns the kernel reads."""
    if isinstance(hash32, torch.Tensor):
        h = hash32.to(device=dev, dtype=torch.int64)
    else:
        h = torch.from_numpy(np.ascontiguousarray(np.asarray(hash32).astype(np.int64))).to(dev)
    return (h & 0xFFFFFFFF).to(torch.int32).contiguous()   # wraps: the low 32 bits


def _bytes_dev(a: np.ndarray, dev) -> torch.Tensor:
    """A device copy of a byte pool; one spare byte so that an empty pool still
    has an address."""
    t = torch.zeros(a.shape[0] + 1, dtype=torch.uint8, device=dev)
    if a.shape[0]:
        t[: a.shape[0]] = torch.from_numpy(a.copy() if not a.flags.writeable else a).to(dev)
    return t


def _launch_hash(user, item, utab, itab, keep, out) -> None:
    """bbgr_md5_pair_hash on device tensors; (data, offsets) device pairs."""
    call("bbgr_md5_pair_hash", user.numel(), ptr(user), ptr(item), ptr(utab[0]), ptr(utab[1]),
         utab[1].numel() - 1, ptr(itab[0]), ptr(itab[1]), itab[1].numel() - 1, ptr(keep),
         ptr(out), stream_handle())


def pair_hash32(user, item, user_ids: IdTable, item_ids: IdTable, device="cuda", *,
                keep=None, out=None) -> torch.Tensor:
    """int64 [n] on the device: per record ``int(md5(f"{uid}|{iid}")[:8], 16)``
    with the ids of ``user[e]`` / ``item[e]``. ``keep`` (optional mask) skips
    records: their entry of ``out`` (an optional uint32-as-int32 [n] device
    buffer, the kernel's own output) stays as it was, and reads 0 without
    ``out``."""
    device = _device(device, "pair_hash32")
    ud, uo = _host_table(user_ids, "user_ids")
    idt, io = _host_table(item_ids, "item_ids")
    n = _check_columns(user, item, uo.shape[0] - 1, io.shape[0] - 1, keep=keep)
    _lib.require_gpu()
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        raw = torch.zeros(n, dtype=torch.int32, device=dev) if out is None else out
        if raw.dtype != torch.int32 or raw.numel() != n or not raw.is_contiguous():
            raise ValueError("out must be a contiguous int32 [n] device tensor")
        if n:
            utab = (_bytes_dev(ud, dev), torch.from_numpy(uo).to(dev))
            itab = (_bytes_dev(idt, dev), torch.from_numpy(io).to(dev))
            k = None if keep is None else _dev(keep, dev, torch.bool).view(torch.uint8)
            _launch_hash(_dev(user, dev, torch.int32), _dev(item, dev, torch.int32), utab, itab,
                         k, raw)
        return raw.long() & 0xFFFFFFFF


def _run_split(user, item, positive, rating, pos_threshold: float, hash_raw, thr, n_users: int,
               n_items: int, user_map, item_map, user_src, item_src, edges, counts) -> None:
    """bbgr_split_edges on device tensors (hash_raw: the 32 bits as int32)."""
    a = _lib.SplitArgs()
    a.n, a.n_users, a.n_items = user.numel(), n_users, n_items
    a.user, a.item = ptr(user), ptr(item)
    a.positive, a.rating, a.pos_threshold = ptr(positive), ptr(rating), pos_threshold
    a.hash32, a.thr_train, a.thr_val = ptr(hash_raw), thr[0], thr[1]
    a.user_map, a.item_map = ptr(user_map), ptr(item_map)
    a.user_src, a.item_src = ptr(user_src), ptr(item_src)
    a.edges, a.ld_edges, a.counts = ptr(edges), edges.stride(0), ptr(counts)
    _lib.call_with_workspace("bbgr_split_edges", ctypes.byref(a), device=user.device)


def split_interactions(user, item, rating, user_ids: IdTable, item_ids: IdTable, *,
                       pos_rating_threshold: float = 4.0, train_p: float = 0.8,
                       val_p: float = 0.1, device="cuda", hash32=None) -> InteractionSplit:
    """The split of the records ``(user[e], item[e], rating[e])`` (module
    docstring). ``hash32`` (optional, [n] integers in [0, 2^32)) replaces the
    md5 launch: a caller's own hash. A positive is ``float(float32(rating)) >=
    pos_rating_threshold``, compared exactly. Raises ValueError, before the device is
    touched, for ids outside the tables, column lengths that differ, n >=
    2^31 - 1, offsets that do not start at 0 or decrease, and ``train_p``,
    ``val_p`` or their sum outside [0, 1]."""
    device = _device(device, "split_interactions")
    thr = split_thresholds(train_p, val_p)
    ud, uo = _host_table(user_ids, "user_ids")
    idt, io = _host_table(item_ids, "item_ids")
    U, I = uo.shape[0] - 1, io.shape[0] - 1
    n = _check_columns(user, item, U, I, rating=rating, hash32=hash32)
    _lib.require_gpu()
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        i32 = dict(dtype=torch.int32, device=dev)
        edges = torch.empty(2, max(n, 1), **i32)
        user_src, item_src = torch.empty(max(U, 1), **i32), torch.empty(max(I, 1), **i32)
        counts = torch.zeros(5, dtype=torch.int64, device=dev)
        if n:
            u, it = _dev(user, dev, torch.int32), _dev(item, dev, torch.int32)
            r = _dev(rating, dev, torch.float32)
            pos_thr = _threshold_f32(pos_rating_threshold)
            if hash32 is None:
                h = torch.empty(n, **i32)
                utab = (_bytes_dev(ud, dev), torch.from_numpy(uo).to(dev))
                itab = (_bytes_dev(idt, dev), torch.from_numpy(io).to(dev))
                # only the positives are hashed: the split reads no other entry
                keep = (r >= pos_thr).view(torch.uint8)
                _launch_hash(u, it, utab, itab, keep, h)
            else:
                h = _hash_raw(hash32, dev)
            _run_split(u, it, None, r, pos_thr, h, thr, U, I,
                       torch.empty(U, **i32), torch.empty(I, **i32), user_src, item_src, edges,
                       counts)
        e_tr, e_va, e_te, n_u, n_i = (int(v) for v in counts.tolist())   # the one host read
        return InteractionSplit(edges[:, :e_tr], edges[:, e_tr:e_tr + e_va],
                                edges[:, e_tr + e_va:e_tr + e_va + e_te], user_src[:n_u],
                                item_src[:n_i], n_u, n_i,
                                {"train": e_tr, "val": e_va, "test": e_te})


def _ids_in_order(ids, src) -> dict:
    """{id string: new index} in new-index order; ``ids`` an IdTable or a
    sequence / dict of str in old-id order."""
    src = src.cpu().numpy() if isinstance(src, torch.Tensor) else np.asarray(src)
    if isinstance(ids, IdTable):
        data, off = _host_table(ids, "ids")
        raw = data.tobytes()
        return {raw[off[o]:off[o + 1]].decode("utf-8"): k for k, o in enumerate(src.tolist())}
    names = list(ids)
    return {names[o]: k for k, o in enumerate(src.tolist())}


def save_split(split: InteractionSplit, out_dir, user_ids, item_ids) -> None:
    """``npy/{train,val,test}_edges.npy`` (int32 [2, E]) and
    ``model/{user2idx,item2idx}.pkl`` (plain dicts in first-appearance order)
    under ``out_dir``: the files ``build_graph_from_jsonl`` leaves, which the
    reference's ``main()`` and ``ingest.load_edges_npy`` read. ``user_ids`` /
    ``item_ids``: the id tables (or sequences of str) the split was made with."""
    out = Path(out_dir)
    (out / "npy").mkdir(parents=True, exist_ok=True)
    (out / "model").mkdir(parents=True, exist_ok=True)
    for name in ("train", "val", "test"):
        e = getattr(split, name)
        e = e.cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e)
        np.save(out / "npy" / f"{name}_edges.npy", np.ascontiguousarray(e, dtype=np.int32))
    for name, ids, src in (("user2idx", user_ids, split.user_src),
                           ("item2idx", item_ids, split.item_src)):
        with open(out / "model" / f"{name}.pkl", "wb") as f:
            pickle.dump(_ids_in_order(ids, src), f, protocol=pickle.HIGHEST_PROTOCOL)
