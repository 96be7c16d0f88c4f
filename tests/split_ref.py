"""Host restatement of what bbgr.split computes: is_positive_interaction,
split_bucket and the two passes of build_graph_from_jsonl
(Version-2/lighgcn_cu_pop.py:96-116, :227-303) over columns and id lists, in
plain Python with hashlib. Everything is integer: the reference for
tests/test_split_host.py and tests/test_gpu_split.py, compared by equality.
A helper, not a test module."""
import hashlib

import numpy as np


def hash32(uid: str, iid: str) -> int:
    """int(h[:8], 16) of split_bucket."""
    return int(hashlib.md5(f"{uid}|{iid}".encode("utf-8")).hexdigest()[:8], 16)


def bucket_of(h: int, train_p: float = 0.8, val_p: float = 0.1) -> str:
    """split_bucket from the 32-bit value on."""
    x = h / 0xFFFFFFFF
    if x < train_p:
        return "train"
    elif x < train_p + val_p:
        return "val"
    return "test"


def is_positive(rating, threshold: float = 4.0) -> bool:
    return float(rating) >= threshold


def pair_hashes(user, item, user_ids, item_ids) -> np.ndarray:
    """int64 [n]: the hash of every record's pair of id strings."""
    return np.asarray([hash32(user_ids[u], item_ids[i])
                       for u, i in zip(np.asarray(user).tolist(), np.asarray(item).tolist())],
                      np.int64).reshape(-1)


def split(user, item, rating, user_ids=None, item_ids=None, *, threshold: float = 4.0,
          train_p: float = 0.8, val_p: float = 0.1, hashes=None) -> dict:
    """The two passes over the records (user[e], item[e], rating[e]) in file
    order; `hashes` (per record) stands in for the md5 of the id strings.
    Returns train / val / test as int32 [2, E], user_src / item_src (the old id
    of every new id) as int32 and the counts."""
    user, item = np.asarray(user).tolist(), np.asarray(item).tolist()
    rating = np.asarray(rating, np.float32).tolist()
    new_u, new_i = {}, {}
    parts = {"train": [], "val": [], "test": []}
    for e, (u, i, r) in enumerate(zip(user, item, rating)):
        if not is_positive(r, threshold):
            continue
        if u not in new_u:
            new_u[u] = len(new_u)
        if i not in new_i:
            new_i[i] = len(new_i)
        h = int(hashes[e]) if hashes is not None else hash32(user_ids[u], item_ids[i])
        parts[bucket_of(h, train_p, val_p)].append((new_u[u], new_i[i]))
    out = {k: np.asarray(v, np.int32).reshape(-1, 2).T.copy() for k, v in parts.items()}
    out["user_src"] = np.asarray(list(new_u), np.int32)
    out["item_src"] = np.asarray(list(new_i), np.int32)
    out["counts"] = {k: len(v) for k, v in parts.items()}
    return out
