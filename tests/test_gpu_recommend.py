"""GPU: recommendation lists (bbgr.recommend) against the C oracle.

The checker is oracle.native.full_topk: the same fp32 fma chain per score,
order (score desc, item asc), any even d, any k, any user list. It scores an
excluded item -1e9 where bbgr_recommend drops it, so the expected lists are the
oracle's with every entry of score <= -1e8 replaced by (-1, -inf); the inputs
keep every real score inside +-0.09 d, and inside +-2 but for the plain table
at d = 256 (asserted). The oracle gets the TRUE-width tables; ids and scores
compare bit for bit.

Inputs: U = 300 users, I = 1500 items (no multiple of a tile; at this user
count the item range splits three ways, so the merge kernel combines six
lists), 257 listed users (one over a 256-user workgroup; permuted, one
duplicate, user 7 among them), exclusion rows of 0-39 random items (sorted,
duplicates kept, every 11th row empty), user 7 excluding all but 5 items.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bbgr.graph import BipartiteGraph, Csr  # noqa: E402
from bbgr.synthetic import synthetic_credibility, synthetic_edges  # noqa: E402
from oracle import native as N  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402

DEV = "cuda"
U, I = 300, 1500
WIDTHS = (8, 16, 32, 64, 128, 256)
KS_64 = (1, 10, 16, 17, 24, 25, 32, 33, 100, 128)
KS_OTHER = (10, 33, 128)
BOUNDARIES = (16, 24, 32, 48, 64, 96)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rows_to_csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def _exclusion(n_items=I):
    """(indptr, indices, rows): 0-39 random items per user, sorted, duplicates
    kept; every 11th row empty; user 7 excludes all but 5 items."""
    rng = np.random.default_rng(77 + n_items)
    deg = rng.integers(0, 40, U)
    deg[::11] = 0
    rows = [np.sort(rng.integers(0, n_items, int(n))).astype(np.int32) for n in deg]
    keep = rng.choice(n_items, 5, replace=False)
    rows[7] = np.setdiff1d(np.arange(n_items, dtype=np.int32), keep).astype(np.int32)
    ptr, idx = _rows_to_csr(rows)
    _frozen(ptr, idx)
    return ptr, idx, tuple(rows)


@functools.lru_cache(maxsize=None)
def _users():
    rng = np.random.default_rng(5)
    ids = rng.permutation(U)[:256]
    if 7 not in ids:
        ids[0] = 7
    ids = rng.permutation(np.concatenate([ids, ids[3:4]])).astype(np.int64)   # one duplicate
    assert ids.size == 257 and 7 in ids and np.unique(ids).size == 256
    return _frozen(ids)[0]


@functools.lru_cache(maxsize=None)
def _tables(d, kind="plain", n_items=I):
    rng = np.random.default_rng(1000 + d)
    uf = rng.uniform(-0.3, 0.3, (U, d)).astype(np.float32)
    if kind == "plain":
        itf = rng.uniform(-0.3, 0.3, (n_items, d)).astype(np.float32)
    else:   # item j is a copy of row j % 30 of a 30-row base: 50 exact ties per score
        base = rng.uniform(-0.3, 0.3, (30, d)).astype(np.float32)
        itf = np.ascontiguousarray(base[np.arange(n_items) % 30])
    # every real score is far from the oracle's -1e9: |score| <= 0.09 d by the
    # ranges, and inside +-2 for every table but the plain one at d = 256
    # (this generator's largest there is 2.43)
    big = np.abs(uf.astype(np.float64) @ itf.astype(np.float64).T).max()
    assert big <= 0.09 * d and (big < 2.0 or (d, kind) == (256, "plain"))
    return _frozen(uf, itf)


def _expected(ptr, idx, uf, itf, k):
    """The oracle's lists with the -1e9 entries (excluded items) dropped."""
    items, scores = N.full_topk(_users(), ptr, idx, uf, itf, k)
    real = scores > -1e8
    assert (np.abs(scores[real]) <= 0.09 * uf.shape[1]).all()
    # excluded entries sort after every real one: dropping them keeps a prefix
    assert (real[:, :-1] >= real[:, 1:]).all()
    _frozen(items, scores)
    return np.where(real, items, -1), np.where(real, scores, -np.inf).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(d, kind="plain", n_items=I, k=128):
    ptr, idx, _ = _exclusion(n_items)
    return _expected(ptr, idx, *_tables(d, kind, n_items), k)


@functools.lru_cache(maxsize=None)
def _ex_csr(n_items=I):
    ptr, idx, rows = _exclusion(n_items)
    r = np.repeat(np.arange(U, dtype=np.int32), np.diff(ptr))
    c = Csr(r, idx, U, n_items, DEV)
    # the device CSR keeps the rows as given (sorted, duplicates included)
    assert np.array_equal(c.indptr.cpu().numpy(), ptr)
    assert np.array_equal(c.indices.cpu().numpy()[:idx.size], idx)
    return c


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def _check(got, want, k):
    (topk, score), (w_items, w_scores) = got, want
    topk, score = topk.cpu().numpy(), score.cpu().numpy()
    assert topk.shape == score.shape == (w_items.shape[0], k)
    assert topk.dtype == np.int32 and score.dtype == np.float32
    np.testing.assert_array_equal(topk, w_items[:, :k])
    np.testing.assert_array_equal(score.view(np.int32),
                                  np.ascontiguousarray(w_scores[:, :k]).view(np.int32))


PLAIN = [(64, k) for k in KS_64] + [(d, k) for d in WIDTHS if d != 64 for k in KS_OTHER]


@pytest.mark.parametrize("d,k", PLAIN)
def test_recommend_plain_table_bitexact(d, k):
    """(a) every width, k on both sides of each list depth and pass count."""
    from bbgr.recommend import recommend
    uf, itf = _tables(d)
    want = _oracle(d)
    got = recommend(_t(uf), _t(itf), _t(_users(), torch.long), k, exclude=_ex_csr(),
                    return_scores=True)
    _check(got, want, k)
    # user 7 has 5 eligible items: -1 / -inf from position 5
    b7 = int(np.flatnonzero(_users() == 7)[0])
    row, sc = got[0][b7].cpu().numpy(), got[1][b7].cpu().numpy()
    assert (row[:min(k, 5)] >= 0).all() and (row[5:] == -1).all() and np.isneginf(sc[5:]).all()
    # ids only, and a host (indptr, indices) exclusion
    ptr, idx, _ = _exclusion()
    only = recommend(_t(uf), _t(itf), _t(_users(), torch.long), k, exclude=(ptr, idx))
    assert torch.equal(only, got[0])


@pytest.mark.parametrize("d", [64, 256])
def test_recommend_tied_table_bitexact(d):
    """(b) 50 exact ties per score, k = 128: a tie group straddles every
    possible pass boundary, so a continuation pass that compared scores but
    not ids, or dropped / repeated an item at a boundary, shows."""
    from bbgr.recommend import recommend
    uf, itf = _tables(d, "tied")
    w_items, w_scores = want = _oracle(d, "tied")
    for p in BOUNDARIES:
        tied = (w_items[:, p] >= 0) & (w_scores[:, p - 1] == w_scores[:, p])
        print(f"tie across {p}|{p + 1}: {int(tied.sum())} of {tied.size} users")
        assert tied.sum() >= 200
    got = recommend(_t(uf), _t(itf), _t(_users(), torch.long), 128, exclude=_ex_csr(),
                    return_scores=True)
    _check(got, want, 128)


@pytest.mark.parametrize("d", [64, 256])
def test_recommend_item_mask(d):
    """(c) only items j % 3 != 0 are eligible: with the exclusion CSR the
    expected lists are the oracle's with each row united with the ineligible
    items; and the mask alone."""
    from bbgr.recommend import recommend
    k = 33
    uf, itf = _tables(d)
    mask = (np.arange(I) % 3 != 0)
    off = np.flatnonzero(~mask).astype(np.int32)
    _, _, rows = _exclusion()
    users = _t(_users(), torch.long)
    both = _expected(*_rows_to_csr([np.union1d(r, off).astype(np.int32) for r in rows]),
                     uf, itf, k)
    got = recommend(_t(uf), _t(itf), users, k, exclude=_ex_csr(), item_mask=_t(mask, torch.bool),
                    return_scores=True)
    _check(got, both, k)
    assert (got[0].cpu().numpy() % 3 != 0).all()    # (-1 % 3 == 2)
    alone = _expected(*_rows_to_csr([off] * U), uf, itf, k)
    got = recommend(_t(uf), _t(itf), users, k, item_mask=mask.astype(np.uint8),
                    return_scores=True)
    _check(got, alone, k)


def test_recommend_small_catalogue_and_no_users():
    """(d) 40 items (less than one tile), k = 100: every row is padded from
    position 40 - |excluded|; an empty user list gives an empty [0, k]."""
    from bbgr.recommend import recommend
    d, n_items, k = 128, 40, 100
    uf, itf = _tables(d, "plain", n_items)
    want = _oracle(d, "plain", n_items, k)
    got = recommend(_t(uf), _t(itf), _t(_users(), torch.long), k, exclude=_ex_csr(n_items),
                    return_scores=True)
    _check(got, want, k)
    _, _, rows = _exclusion(n_items)
    n_ok = np.array([n_items - np.unique(rows[u]).size for u in _users()])
    assert n_ok[_users() == 7].tolist() == [5]
    assert np.array_equal((got[0].cpu().numpy() >= 0).sum(1), n_ok)
    topk, score = recommend(_t(uf), _t(itf), torch.zeros(0, dtype=torch.long, device=DEV), k,
                            exclude=_ex_csr(n_items), return_scores=True)
    assert topk.shape == score.shape == (0, k) and topk.dtype == torch.int32
    assert recommend(_t(uf), _t(itf), [], k).shape == (0, k)


# ---------------------------------------------------------------------------
# (e) evaluate_ranking
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _split():
    e = synthetic_edges(U, I, 6000, 3, items="zipf")
    rng = np.random.default_rng(3)
    test = rng.random(e.shape[1]) < 0.2
    tr, te = e[:, ~test], e[:, test]
    # every user keeps at least 100 items outside the train row
    assert I - np.bincount(tr[0], minlength=U).max() >= 100
    return _frozen(tr, te)


def _eval_inputs(d):
    tr, te = _split()
    uf, itf = _tables(d)
    pop = np.bincount(tr[1], minlength=I)
    cred = synthetic_credibility(U, 4)
    args = (_t(uf), _t(itf), Csr(tr[0], tr[1], U, I, DEV), Csr(te[0], te[1], U, I, DEV), I, pop,
            int(tr.shape[1]), cred)
    return tr, te, uf, itf, pop, cred, args


@pytest.mark.parametrize("d", [64, 128])
def test_evaluate_ranking_equals_evaluate_full(d):
    """Where every user has max(Ks) eligible items the two protocols are the
    same computation: equal result dictionaries (the sums bit for bit), equal
    lists and scores."""
    from bbgr.evaluation import evaluate_full
    from bbgr.recommend import evaluate_ranking
    *_, args = _eval_inputs(d)
    full = evaluate_full(*args, Ks=(10, 20), return_raw=True)
    rank = evaluate_ranking(*args, Ks=(10, 20), return_raw=True)
    fr, rr = full.pop("_raw"), rank.pop("_raw")
    assert full == rank and full[10]["mode"] == "full"
    assert set(fr) == set(rr)
    for key in ("users", "topk", "groups"):
        assert torch.equal(fr[key], rr[key]), key
    assert torch.equal(fr["topk_score"].view(torch.int32), rr["topk_score"].view(torch.int32))


def test_evaluate_ranking_at_256_vs_metric_loop():
    """d = 256 and K = 50 / 100, which evaluate_full refuses: the metrics are
    the reference's metric loop (oracle evaluate_given_topk) on the oracle's
    lists; float tolerance as tests/test_gpu_eval.py's full-ranking test,
    integer counts exact."""
    from bbgr.recommend import evaluate_ranking
    Ks = (10, 20, 50, 100)
    tr, te, uf, itf, pop, cred, args = _eval_inputs(256)
    res = evaluate_ranking(*args, Ks=Ks, return_raw=True)
    raw = res.pop("_raw")
    users = raw["users"].cpu().numpy()
    tr_ptr, tr_idx = R.edges_to_user_csr(tr, U)
    te_ptr, te_idx = R.edges_to_user_csr(te, U)
    o_items, o_scores = N.full_topk(users, tr_ptr, tr_idx, uf, itf, max(Ks))
    assert (o_scores > -1e8).all()
    np.testing.assert_array_equal(raw["topk"].cpu().numpy(), o_items)
    np.testing.assert_array_equal(raw["topk_score"].cpu().numpy().view(np.int32),
                                  o_scores.view(np.int32))
    flags = raw["groups"].cpu().numpy()
    ref = R.evaluate_given_topk(users, o_items, te_ptr, te_idx, pop, int(tr.shape[1]), I, cred,
                                users[flags & 1 > 0], users[flags & 2 > 0], Ks=Ks)
    for K in Ks:
        for key in ref[K]:
            if key in ("high_users", "low_users"):
                assert res[K][key] == ref[K][key], (K, key)
            else:
                assert res[K][key] == pytest.approx(ref[K][key], rel=1e-9, abs=1e-12), (K, key)
        assert res[K]["mode"] == "full" and res[K]["users_eval"] == users.size


# ---------------------------------------------------------------------------
# (f) callers
# ---------------------------------------------------------------------------
def _model(family, d):
    from bbgr import lightgcn_cu as CU
    from bbgr import lightgcn_cu_pop as V2
    e = synthetic_edges(U, 350, 4000, 17, items="zipf", duplicates=20)
    cred = synthetic_credibility(U, 5)
    torch.manual_seed(d)
    if family == "v2_pop":
        M_ui, M_iu = V2.build_message_passing_mats(e, U, 350, torch.as_tensor(cred), DEV)
        return V2.LightGCN(U, 350, d, 3, M_ui, M_iu).to(DEV), e
    M_ui, M_iu, _ = CU.build_cred_weighted_mats(e, U, 350, cred, DEV)
    return CU.CredLightGCN(U, 350, d, 3, M_ui, M_iu).to(DEV), e


@pytest.mark.parametrize("family,d", [("v2_pop", 16), ("cu_fair", 256)])
def test_recommend_model_reads_the_final_tables(family, d):
    from bbgr.recommend import recommend, recommend_model
    m, e = _model(family, d)
    users = _t(_users(), torch.long)
    ex = Csr(e[0], e[1], U, 350, DEV)
    with torch.no_grad():
        ue, ie = m.final_embeddings() if family == "cu_fair" else m.get_user_item_emb()
    want = recommend(ue, ie, users, 33, exclude=ex, return_scores=True)
    got = recommend_model(m, users, 33, exclude=ex, return_scores=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[0] >= 0).all() and got[0].max() < 350


@pytest.mark.parametrize("order", ["input", "degree"])
def test_trainer_recommend(order):
    from bbgr.recommend import recommend
    from bbgr.trainer import FusedTrainer
    e = synthetic_edges(U, 350, 4000, 17, items="zipf", duplicates=20)
    g = BipartiteGraph(e, U, 350, DEV, vertex_order=order)
    tr = FusedTrainer(g, "v2_pop", cred=synthetic_credibility(U, 5), emb_dim=32, num_layers=2,
                      batch_size=64)
    tr.step()
    users = _t(_users(), torch.long)
    train = Csr(e[0], e[1], U, 350, DEV)    # rows and columns by input id
    want = recommend(*tr.forward(), users, 20, exclude=train, return_scores=True)
    got = tr.recommend(users, 20, return_scores=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # no train item in a list; without the exclusion some user gets one
    has = np.zeros((U, 350), bool)
    has[e[0], e[1]] = True
    lists = got[0].cpu().numpy()
    assert not has[_users()[:, None], lists].any()
    free = tr.recommend(users, 20, exclude_train=False).cpu().numpy()
    assert has[_users()[:, None], free].any()
    assert torch.equal(tr.recommend(users, 20, exclude_train=False),
                       recommend(*tr.forward(), users, 20))


def test_out_of_range_users_raise_and_the_device_stays_healthy():
    from bbgr.recommend import recommend
    uf, itf = _tables(64)
    for bad in ([0, U], [-1, 3]):
        with pytest.raises(ValueError, match="user ids"):
            recommend(_t(uf), _t(itf), _t(bad, torch.long), 10)
    with pytest.raises(ValueError, match="k must be"):
        recommend(_t(uf), _t(itf), _t([0], torch.long), 129)
    got = recommend(_t(uf), _t(itf), _t(_users(), torch.long), 10, exclude=_ex_csr(),
                    return_scores=True)
    torch.cuda.synchronize()
    _check(got, _oracle(64), 10)
