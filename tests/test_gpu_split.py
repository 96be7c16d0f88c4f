"""GPU: bbgr.split (csrc/split.hip) against the host restatement
tests/split_ref.py (Version-2/lighgcn_cu_pop.py:96-116, :227-303). Everything
is integer: every comparison is equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import split_ref as SR  # noqa: E402

DEV = "cuda"
U, I = 300, 200
HUB = 2500             # records of the hub user and of the hub item
TILE = 2048            # records per workgroup of the scans (SPLIT_TILE)
SCAN_STEP = 1024       # tiles per step of the tile-count scan
SENTINEL = -7
PAD = 96
# id bytes of a pair (user + item; the message is one byte longer): each side of the
# one-to-two and two-to-three block edges whichever of the two lengths is counted
PAIR_BYTES = [0, 1, 53, 54, 55, 56, 57, 62, 63, 64, 65, 117, 118, 119, 120, 121, 200]
BOUNDARY_HASHES = [0, 3435973835, 3435973836, 3865470565, 3865470566, 0xFFFFFFFF]


def _split_mod():
    import bbgr.split as S
    return S


def _ascii(rng, n: int) -> str:
    return "".join(chr(c) for c in rng.integers(33, 127, n))


# -- 1. the hash -------------------------------------------------------------------------
def _length_case():
    """One record per (pair bytes, cut): the user id takes `cut` of the bytes."""
    rng = np.random.default_rng(5)
    users, items = [], []
    for total in PAIR_BYTES:
        for cut in sorted({0, total, total // 2, int(rng.integers(0, total + 1)), min(total, 3)}):
            users.append(_ascii(rng, cut))
            items.append(_ascii(rng, total - cut))
    return users, items


def _check_hash(user_ids, item_ids, user, item):
    S = _split_mod()
    got = S.pair_hash32(user, item, S.id_table(user_ids), S.id_table(item_ids), DEV)
    assert got.dtype == torch.int64 and got.is_cuda
    want = SR.pair_hashes(user, item, user_ids, item_ids)
    assert np.array_equal(got.cpu().numpy(), want)


def test_hash_at_every_block_edge():
    users, items = _length_case()
    assert "" in users and "" in items
    k = np.arange(len(users), dtype=np.int32)
    _check_hash(users, items, k, k)
    # and crossed: record e pairs user e with another item
    _check_hash(users, items, k, k[::-1].copy())


def test_hash_of_multi_byte_utf8_ids():
    users = ["ü", "日本語のユーザー", "\U0001F600\U0001F601", "aé日\U0001F600", "ÀÉÎÕÜ" * 11,
             "plain", "語" * 18 + "x", "\U0001F680" * 14]
    items = ["é", "商品", "\U0001F4E6", "B0é日\U0001F600", "ß" * 27, "B00005N7P0", "語", "\U0001F680" * 16]
    rng = np.random.default_rng(6)
    user = rng.integers(0, len(users), 64).astype(np.int32)
    item = rng.integers(0, len(items), 64).astype(np.int32)
    _check_hash(users, items, user, item)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_hash_at_workgroup_sizes(n):
    rng = np.random.default_rng(n)
    users = ["AE" + _ascii(rng, 26) for _ in range(40)]     # the dataset's shapes
    items = ["B0" + _ascii(rng, 8) for _ in range(30)]
    _check_hash(users, items, rng.integers(0, 40, n).astype(np.int32),
                rng.integers(0, 30, n).astype(np.int32))


def test_hash_keep_mask_leaves_poisoned_outputs_untouched():
    S = _split_mod()
    rng = np.random.default_rng(8)
    n = 700
    users = [_ascii(rng, int(k)) for k in rng.integers(0, 70, 50)]
    items = [_ascii(rng, int(k)) for k in rng.integers(0, 70, 50)]
    user = rng.integers(0, 50, n).astype(np.int32)
    item = rng.integers(0, 50, n).astype(np.int32)
    keep = rng.random(n) < 0.5
    poison = torch.full((n + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    got = S.pair_hash32(user, item, S.id_table(users), S.id_table(items), DEV, keep=keep,
                        out=poison[:n]).cpu().numpy()
    want = SR.pair_hashes(user, item, users, items)
    assert np.array_equal(got[keep], want[keep])
    assert (got[~keep] == 0x5A5A5A5A).all()
    assert (poison[n:] == 0x5A5A5A5A).all()


# -- comparison against split_ref ----------------------------------------------------------
def _assert_split(got, ref):
    for name in ("train", "val", "test"):
        g = getattr(got, name)
        assert g.dtype == torch.int32 and g.dim() == 2 and g.shape[0] == 2 and g.is_cuda
        assert np.array_equal(g.cpu().numpy(), ref[name]), name
    assert np.array_equal(got.user_src.cpu().numpy(), ref["user_src"])
    assert np.array_equal(got.item_src.cpu().numpy(), ref["item_src"])
    assert got.num_users == len(ref["user_src"]) and got.num_items == len(ref["item_src"])
    assert got.counts == ref["counts"]


# -- 2. the boundaries -------------------------------------------------------------------
def _boundary_split(**kw):
    S = _split_mod()
    n = len(BOUNDARY_HASHES)
    ids = S.id_table([f"id{k}" for k in range(n)])
    k = np.arange(n, dtype=np.int32)
    rating = np.full(n, 5.0, np.float32)
    got = S.split_interactions(k, k, rating, ids, ids, device=DEV,
                               hash32=np.asarray(BOUNDARY_HASHES, np.int64), **kw)
    _assert_split(got, SR.split(k, k, rating, hashes=BOUNDARY_HASHES, **kw))
    return got


def test_boundaries_with_the_default_probabilities():
    """train, train, val, val, test, test; a float32 division would move the
    second and the fourth."""
    got = _boundary_split()
    assert got.train.tolist() == [[0, 1], [0, 1]]
    assert got.val.tolist() == [[2, 3], [2, 3]]
    assert got.test.tolist() == [[4, 5], [4, 5]]
    assert np.float32(3435973835) / np.float32(0xFFFFFFFF) >= np.float32(0.8)
    assert np.float32(3865470565) / np.float32(0xFFFFFFFF) >= np.float32(0.9)


@pytest.mark.parametrize("train_p,val_p", [(0.5, 0.25), (1.0, 0.0), (0.0, 0.0)])
def test_boundaries_with_other_probabilities(train_p, val_p):
    _boundary_split(train_p=train_p, val_p=val_p)


# -- 3. the whole split ------------------------------------------------------------------
def _main_dump():
    """About 6,000 records over U users and I items in permuted file order: a
    hub user (7) and a hub item (3), repeated pairs, users 280.. and items 190..
    without a positive record, user U - 1 and item I - 1 without any record."""
    rng = np.random.default_rng(2025)
    n_base = 1200
    user = [rng.integers(0, 280, n_base), np.full(HUB, 7), rng.integers(0, 280, HUB),
            rng.integers(280, U - 1, 60), rng.integers(0, 280, 60)]
    item = [rng.integers(0, 190, n_base), rng.integers(0, 190, HUB), np.full(HUB, 3),
            rng.integers(0, 190, 60), rng.integers(190, I - 1, 60)]
    user, item = np.concatenate(user), np.concatenate(item)
    rating = rng.choice(np.asarray([1, 3.5, 4, 4.5, 5], np.float32), user.shape[0])
    rating[n_base + 2 * HUB:] = rng.choice(np.asarray([1, 3.5], np.float32), 120)
    rep = rng.integers(0, user.shape[0], 150)               # repeated pairs, own ratings
    user, item = np.concatenate([user, user[rep]]), np.concatenate([item, item[rep]])
    rating = np.concatenate([rating, rng.choice(np.asarray([4, 5], np.float32), 150)])
    rating[np.isin(user, np.arange(280, U)) | np.isin(item, np.arange(190, I))] = 3.5
    order = rng.permutation(user.shape[0])
    names = np.random.default_rng(1)
    user_ids = ["AE" + _ascii(names, 26) for _ in range(U)]
    item_ids = ["B0" + _ascii(names, 8) for _ in range(I)]
    user_ids[11], item_ids[5] = "ユーザー" + _ascii(names, 40), ""      # two blocks; an empty id
    return (user[order].astype(np.int32), item[order].astype(np.int32),
            rating[order].astype(np.float32), user_ids, item_ids)


@pytest.fixture(scope="module")
def dump():
    S = _split_mod()
    user, item, rating, user_ids, item_ids = _main_dump()
    return dict(user=user, item=item, rating=rating, user_ids=user_ids, item_ids=item_ids,
                ut=S.id_table(user_ids), it=S.id_table(item_ids))


def _run(d, n=None, **kw):
    S = _split_mod()
    n = len(d["user"]) if n is None else n
    rating = kw.pop("rating", d["rating"])
    got = S.split_interactions(d["user"][:n], d["item"][:n], rating[:n], d["ut"], d["it"],
                               device=DEV, **kw)
    if "pos_rating_threshold" in kw:
        kw["threshold"] = kw.pop("pos_rating_threshold")
    ref = SR.split(d["user"][:n], d["item"][:n], rating[:n], d["user_ids"], d["item_ids"], **kw)
    return got, ref


def test_main_case(dump):
    got, ref = _run(dump)
    n = len(dump["user"])
    assert 5900 < n < 6600
    # the case has what it says: first appearance differs from id order, ids without a
    # positive record, repeated pairs, all three buckets
    assert not np.array_equal(ref["user_src"], np.sort(ref["user_src"]))
    assert len(ref["user_src"]) < U - 1 and len(ref["item_src"]) < I - 1
    pairs = np.concatenate([ref["train"], ref["val"], ref["test"]], axis=1).T
    assert len(np.unique(pairs, axis=0)) < len(pairs)
    assert min(ref["counts"].values()) > 100
    _assert_split(got, ref)
    # one buffer: the three parts are views of it, side by side
    assert got.train.data_ptr() + 4 * got.counts["train"] == got.val.data_ptr()
    assert got.val.data_ptr() + 4 * got.counts["val"] == got.test.data_ptr()


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 4097])
def test_prefixes_at_tile_edges(dump, n):
    _assert_split(*_run(dump, n))


@pytest.mark.parametrize("n", [SCAN_STEP * TILE, SCAN_STEP * TILE + 1])
def test_tile_count_scan_past_one_step(n):
    """More tiles than one step of the tile-count scan holds, with a caller's hash."""
    S = _split_mod()
    rng = np.random.default_rng(n)
    ids = S.id_table([f"{k}" for k in range(5000)])
    user = rng.integers(0, 5000, n).astype(np.int32)
    item = rng.integers(0, 5000, n).astype(np.int32)
    rating = rng.choice(np.asarray([3.5, 4, 5], np.float32), n, p=[0.7, 0.15, 0.15])
    hashes = rng.integers(0, 2**32, n, dtype=np.int64)
    got = S.split_interactions(user, item, rating, ids, ids, device=DEV, hash32=hashes)
    _assert_split(got, SR.split(user, item, rating, hashes=hashes.tolist()))


def test_no_positives_at_all(dump):
    rating = np.full_like(dump["rating"], 3.5)
    got, ref = _run(dump, rating=rating)
    _assert_split(got, ref)
    assert got.num_users == 0 and got.num_items == 0
    assert got.counts == {"train": 0, "val": 0, "test": 0}
    for t in (got.train, got.val, got.test):
        assert tuple(t.shape) == (2, 0)
    assert got.user_src.numel() == 0 and got.item_src.numel() == 0


def test_all_positives(dump):
    got, ref = _run(dump, rating=np.full_like(dump["rating"], 4.0))
    assert sum(ref["counts"].values()) == len(dump["user"])
    _assert_split(got, ref)


def test_the_positive_test_is_exact_on_the_float32_rating(dump):
    """3.3 as float32 lies below the double 3.3: not positive at that threshold."""
    rating = np.where(dump["rating"] >= 4, np.float32(3.3), np.float32(1)).astype(np.float32)
    got, ref = _run(dump, rating=rating, pos_rating_threshold=3.3)
    assert sum(ref["counts"].values()) == 0
    _assert_split(got, ref)
    got, ref = _run(dump, rating=rating, pos_rating_threshold=float(np.float32(3.3)))
    assert sum(ref["counts"].values()) > 1000
    _assert_split(got, ref)


def _raw_call(d, hash_raw, pad: int):
    """bbgr_split_edges with every output a leading view of a larger
    sentinel-filled buffer; returns the buffers."""
    S = _split_mod()
    n = len(d["user"])
    i32 = dict(dtype=torch.int32, device=DEV)
    big = {"user_map": torch.full((U + pad,), SENTINEL, **i32),
           "item_map": torch.full((I + pad,), SENTINEL, **i32),
           "user_src": torch.full((U + pad,), SENTINEL, **i32),
           "item_src": torch.full((I + pad,), SENTINEL, **i32),
           "edges": torch.full((2 * n + pad,), SENTINEL, **i32),
           "counts": torch.full((5 + pad,), SENTINEL, dtype=torch.int64, device=DEV)}
    S._run_split(torch.from_numpy(d["user"]).to(DEV), torch.from_numpy(d["item"]).to(DEV), None,
                 torch.from_numpy(d["rating"]).to(DEV), 4.0, hash_raw, S.split_thresholds(), U, I,
                 big["user_map"][:U], big["item_map"][:I], big["user_src"][:U],
                 big["item_src"][:I], big["edges"][:2 * n].view(2, n), big["counts"][:5])
    torch.cuda.synchronize()
    return big


def test_outputs_stay_inside_their_views_and_two_calls_agree(dump):
    S = _split_mod()
    n = len(dump["user"])
    ref = SR.split(dump["user"], dump["item"], dump["rating"], dump["user_ids"], dump["item_ids"])
    h = S.pair_hash32(dump["user"], dump["item"], dump["ut"], dump["it"], DEV).to(torch.int32)
    a, b = _raw_call(dump, h, PAD), _raw_call(dump, h, PAD)
    for name in a:
        assert torch.equal(a[name], b[name]), name            # the same bits
    e_tr, e_va, e_te, n_u, n_i = a["counts"][:5].tolist()
    assert {"train": e_tr, "val": e_va, "test": e_te} == ref["counts"]
    assert (n_u, n_i) == (len(ref["user_src"]), len(ref["item_src"]))
    assert (a["counts"][5:] == SENTINEL).all()
    assert np.array_equal(a["user_src"][:n_u].cpu().numpy(), ref["user_src"])
    assert np.array_equal(a["item_src"][:n_i].cpu().numpy(), ref["item_src"])
    assert (a["user_src"][n_u:] == SENTINEL).all() and (a["item_src"][n_i:] == SENTINEL).all()
    assert (a["user_map"][U:] == SENTINEL).all() and (a["item_map"][I:] == SENTINEL).all()
    # the maps invert the lists; an id without a positive record maps to -1
    umap = a["user_map"][:U].cpu().numpy()
    assert np.array_equal(umap[ref["user_src"]], np.arange(n_u))
    assert (np.delete(umap, ref["user_src"]) == -1).all() and (umap == -1).sum() == U - n_u
    imap = a["item_map"][:I].cpu().numpy()
    assert np.array_equal(imap[ref["item_src"]], np.arange(n_i))
    assert (imap == -1).sum() == I - n_i
    edges = a["edges"][:2 * n].view(2, n)
    want = np.concatenate([ref["train"], ref["val"], ref["test"]], axis=1)
    P = want.shape[1]
    assert np.array_equal(edges[:, :P].cpu().numpy(), want)
    assert (edges[:, P:] == SENTINEL).all() and (a["edges"][2 * n:] == SENTINEL).all()


# -- 4. joined to the recommender ----------------------------------------------------------
def test_split_feeds_the_recommender(dump):
    from bbgr.lightgcn_cu_pop import LightGCN, build_message_passing_mats
    S = _split_mod()
    split = S.split_interactions(dump["user"], dump["item"], dump["rating"], dump["ut"],
                                 dump["it"], device=DEV)
    cred_all = torch.from_numpy(np.random.default_rng(3).random(U).astype(np.float32))
    cred = split.cred(cred_all)
    assert cred.shape == (split.num_users,) and cred.is_cuda
    assert torch.equal(cred.cpu(), cred_all[split.user_src.cpu().long()])
    M_ui, M_iu = build_message_passing_mats(split.train.cpu().numpy(), split.num_users,
                                            split.num_items, cred, DEV)
    torch.manual_seed(0)
    m = LightGCN(split.num_users, split.num_items, 64, 2, M_ui, M_iu).to(DEV)
    uf, itf = m.propagate()
    uf, itf = uf.detach().double().cpu().numpy(), itf.detach().double().cpu().numpy()
    assert uf.shape == (split.num_users, 64) and itf.shape == (split.num_items, 64)
    assert np.isfinite(uf).all() and np.isfinite(itf).all() and np.abs(uf).max() > 0
