"""CPU: the host half of bbgr.split: the integer thresholds against Python's
own double division, the id tables, the files save_split leaves, and every
ValueError, raised before the device is touched (no GPU here)."""
import pickle

import numpy as np
import pytest
import torch

import split_ref as SR  # noqa: E402
from bbgr import ingest
from bbgr.split import (IdTable, InteractionSplit, id_table, pair_hash32, save_split,
                        split_interactions, split_thresholds)

DENOM = 0xFFFFFFFF


def test_default_thresholds():
    assert split_thresholds() == (3435973836, 3865470566)
    assert split_thresholds(0.8, 0.1) == (3435973836, 3865470566)
    # 0.8 * 0xFFFFFFFF is the integer 3435973836 exactly, and x < 0.8 is false there: val
    assert 3435973836 / DENOM == 0.8 and SR.bucket_of(3435973836) == "val"
    assert SR.bucket_of(3435973835) == "train"
    assert SR.bucket_of(3865470565) == "val" and SR.bucket_of(3865470566) == "test"


def _pairs():
    rng = np.random.default_rng(11)
    out = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.8, 0.1)]
    while len(out) < 205:
        a, b = rng.random(), rng.random()
        if a + b <= 1.0:
            out.append((float(a), float(b)))
    return out


@pytest.mark.parametrize("chunk", range(5))
def test_thresholds_are_the_boundaries_of_pythons_division(chunk):
    """v = thr - 1 is below p and v = thr is not, for both lines of split_bucket."""
    for train_p, val_p in _pairs()[chunk::5]:
        thr = split_thresholds(train_p, val_p)
        assert 0 <= thr[0] <= thr[1] <= 2**32
        for t, p in zip(thr, (train_p, train_p + val_p)):
            if t > 0:
                assert (t - 1) / DENOM < p, (train_p, val_p, t)
            if t < 2**32:
                assert not (t / DENOM < p), (train_p, val_p, t)
            else:   # every 32-bit value is below p
                assert DENOM / DENOM < p


def test_threshold_extremes():
    assert split_thresholds(0.0, 0.0) == (0, 0)
    assert split_thresholds(1.0, 0.0) == (DENOM, DENOM)     # only x == 1.0 is not below 1.0
    assert split_thresholds(0.0, 1.0) == (0, DENOM)
    assert split_thresholds(0.5, 0.5) == (2**31, DENOM)


@pytest.mark.parametrize("train_p,val_p,name", [
    (-0.1, 0.5, "train_p"), (1.5, 0.0, "train_p"), (0.5, -0.1, "val_p"), (0.2, 1.1, "val_p"),
    (0.8, 0.3, r"train_p \+ val_p"), (float("nan"), 0.1, "train_p"),
])
def test_probabilities_outside_the_unit_interval(train_p, val_p, name):
    with pytest.raises(ValueError, match=name):
        split_thresholds(train_p, val_p)


def test_id_table_round_trips_multi_byte_ids():
    ids = ["AE2", "", "ü", "日本語", "x\U0001F600y", "plain-ascii-0123456789"]
    t = id_table(ids)
    assert len(t) == len(ids) and t.data.dtype == np.uint8 and t.offsets.dtype == np.int64
    assert t.offsets[0] == 0 and t.offsets[-1] == t.data.shape[0]
    raw = t.data.tobytes()
    back = [raw[t.offsets[k]:t.offsets[k + 1]].decode("utf-8") for k in range(len(ids))]
    assert back == ids
    assert [int(v) for v in np.diff(t.offsets)] == [3, 0, 2, 9, 6, 22]
    # a dict in first-appearance order is the table of its index
    d = {"b": 0, "a": 1, "ç": 2}
    assert id_table(d).data.tobytes() == "baç".encode("utf-8")
    assert len(id_table([])) == 0 and id_table([]).offsets.tolist() == [0]


def test_save_split_writes_the_reference_files(tmp_path):
    """A hand-made split with CPU tensors: the files load through
    ingest.load_edges_npy and pickle; the dicts are {id: k} in order."""
    user_ids, item_ids = ["u0", "ü1", "u2", "u3"], ["i0", "i1", "日2"]
    e = torch.tensor([[0, 1, 1, 2, 0], [0, 0, 1, 2, 2]], dtype=torch.int32)
    s = InteractionSplit(e[:, :3], e[:, 3:4], e[:, 4:], torch.tensor([2, 0, 3], dtype=torch.int32),
                         torch.tensor([1, 2, 0], dtype=torch.int32), 3, 3,
                         {"train": 3, "val": 1, "test": 1})
    for k, (uid, iid) in enumerate(((id_table(user_ids), id_table(item_ids)), (user_ids, item_ids),
                                    (dict.fromkeys(user_ids), dict.fromkeys(item_ids)))):
        out = tmp_path / f"out{k}"
        save_split(s, out, uid, iid)
        for name, want in (("train", e[:, :3]), ("val", e[:, 3:4]), ("test", e[:, 4:])):
            got = ingest.load_edges_npy(out / "npy" / f"{name}_edges.npy")
            assert got.dtype == np.int32 and np.array_equal(got, want.numpy())
        with open(out / "model" / "user2idx.pkl", "rb") as f:
            u2i = pickle.load(f)
        with open(out / "model" / "item2idx.pkl", "rb") as f:
            i2i = pickle.load(f)
        assert type(u2i) is dict and list(u2i.items()) == [("u2", 0), ("u0", 1), ("u3", 2)]
        assert type(i2i) is dict and list(i2i.items()) == [("i1", 0), ("日2", 1), ("i0", 2)]


def test_cred_gathers_by_user_src():
    s = InteractionSplit(None, None, None, torch.tensor([2, 0, 3], dtype=torch.int32),
                         torch.tensor([0], dtype=torch.int32), 3, 1, {})
    cred_all = np.asarray([0.1, 0.2, 0.3, 0.4], np.float32)
    assert s.cred(cred_all).tolist() == pytest.approx([0.3, 0.1, 0.4])
    assert s.cred(torch.from_numpy(cred_all)).dtype == torch.float32


# -- ValueErrors, before the device is touched -------------------------------------------
UT, IT = id_table(["a", "b", "c"]), id_table(["x", "y"])
Z = np.zeros(3, np.int32)
R = np.full(3, 5.0, np.float32)


def _both(match, user=Z, item=Z, rating=R, ut=UT, it=IT, **kw):
    with pytest.raises(ValueError, match=match):
        split_interactions(user, item, rating, ut, it, **kw)
    if not kw:
        with pytest.raises(ValueError, match=match):
            pair_hash32(user, item, ut, it)


def test_ids_outside_the_tables():
    _both(r"user id out of range: \[0, 3\]", user=np.asarray([0, 3, 1], np.int32))
    _both("user id out of range", user=np.asarray([0, -1, 1], np.int32))
    _both(r"item id out of range: \[0, 2\]", item=np.asarray([2, 0, 1], np.int32))
    _both("item id out of range", item=torch.tensor([0, -5, 1], dtype=torch.int32))


def test_column_length_mismatches():
    _both("column item: expected 3 entries, got 2", item=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="column rating: expected 3 entries, got 4"):
        split_interactions(Z, Z, np.ones(4, np.float32), UT, IT)
    with pytest.raises(ValueError, match="column hash32: expected 3 entries, got 1"):
        split_interactions(Z, Z, R, UT, IT, hash32=np.zeros(1, np.int64))
    with pytest.raises(ValueError, match="column keep"):
        pair_hash32(Z, Z, UT, IT, keep=np.ones(5, bool))


def test_too_many_records():
    class Huge:
        ndim, shape = 1, (2**31 - 1,)
    with pytest.raises(ValueError, match=r"n must be < 2\^31 - 1"):
        split_interactions(Huge(), Huge(), Huge(), UT, IT)
    with pytest.raises(ValueError, match=r"n must be < 2\^31 - 1"):
        pair_hash32(Huge(), Huge(), UT, IT)


def test_bad_offsets():
    data = np.frombuffer(b"abc", np.uint8)
    _both("user_ids.offsets must start at 0", ut=IdTable(data, np.asarray([1, 2, 3, 3], np.int64)))
    _both("user_ids.offsets must not decrease",
          ut=IdTable(data, np.asarray([0, 2, 1, 3], np.int64)))
    _both("item_ids.offsets must not decrease", it=IdTable(data, np.asarray([0, 3, 2], np.int64)))
    _both("item_ids.offsets end at 4, past the 3 bytes",
          it=IdTable(data, np.asarray([0, 2, 4], np.int64)))
    _both("user_ids.offsets must be an int64", ut=IdTable(data, np.asarray([0, 1, 2, 3], np.int32)))
    _both("user_ids.data must be a uint8", ut=IdTable(data.astype(np.int8), UT.offsets))


def test_bad_probabilities_reach_split_interactions():
    _both("train_p", train_p=1.2)
    _both("val_p", val_p=-0.5)
    _both(r"train_p \+ val_p", train_p=0.7, val_p=0.4)


def test_a_non_gpu_device_is_refused():
    with pytest.raises(ValueError, match="runs on the GPU; there is no CPU fallback"):
        split_interactions(Z, Z, R, UT, IT, device="cpu")
    with pytest.raises(ValueError, match="runs on the GPU; there is no CPU fallback"):
        pair_hash32(Z, Z, UT, IT, device="cpu")


def test_split_ref_is_the_reference_on_a_case_worked_by_hand():
    """Two users, two items, one negative: numbering by first appearance among
    the positives, buckets by the injected hashes."""
    out = SR.split([1, 0, 1, 0], [1, 1, 0, 0], [5, 3, 4, 4.5],
                   hashes=[0, 0, 3435973836, 0xFFFFFFFF])
    assert out["user_src"].tolist() == [1, 0] and out["item_src"].tolist() == [1, 0]
    assert out["train"].tolist() == [[0], [0]] and out["val"].tolist() == [[0], [1]]
    assert out["test"].tolist() == [[1], [1]]
    assert out["counts"] == {"train": 1, "val": 1, "test": 1}
    # md5("") = d41d8cd9..., md5("|") = b99834bc...: the separator is part of the message
    assert SR.hash32("", "") == 0xB99834BC
