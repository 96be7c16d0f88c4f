"""GPU: csrc/features.hip, and bbgr_csr_build as the features call it, at the
edges tests/test_gpu_features.py does not reach: row lengths around
FEAT_LONG_ROW = 512 and around multiples of the workgroup's stride 256, more
long rows than FEAT_LONG_GRID = 256 workgroups, ratings whose double sums
depend on the order, timestamps at epoch scale, the edge kernel's tile tails
with poisoned memory behind every output, the statistics kernel's strided
second trip, and sort keys of one column and of more than 32 bits.

The reference is tests/features_ref.py (Python doubles in file order). A mean
over a row (item_x[:, 0], user columns 3, 5, 6) gets two checks: within 1
float32 ulp of that reference, and |got - m| <= ulp32(m)/2 + (n + 2) 2^-53 |m|
with m = math.fsum(terms) / n: half an ulp for the one rounding to float32,
gamma_(n+2) for a double sum of n non-negative terms in any order and a
division. A float32 accumulator breaks the second check. The largest values
seen on MI355X are in DESIGN 4d."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import features_ref as FR  # noqa: E402

DEV = "cuda"
TAU = FR.TAU_MS
LONG_ROW = 512                   # FEAT_LONG_ROW: longer rows take one workgroup each
LONG_GRID = 256                  # FEAT_LONG_GRID: workgroups striding over the long-row list
STATS_THREADS = 1024 * 256       # the statistics grid: beyond it the strided loop trips again
EPOCH = 1_500_000_000_000        # ms
RATINGS = np.asarray([0.3, 1.1, 2.5, 2.9, 3.7, 4.3, 4.5, 5.0], np.float32)
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025,
           2049]
MEAN_USER_COLS = {3: "deviation", 5: "diversity", 6: "discrepancy"}
EXACT_USER_COLS = [0, 2, 4]
OUTPUT_KEYS = ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
               "helpful_reviews")

# the boundary graph's ids
N_LONG = 300                                   # long users 0..299 and long items 0..299
U_BOUND = I_BOUND = N_LONG                     # one boundary row per entry of LENGTHS
U_THRESH = U_BOUND + len(LENGTHS)              # four 1000-record users
THRESHOLDS = [(700, 1), (300, 0), (699, -1), (301, -1)]     # (helpful records, label)
U_NO_TS, U_FEW_TS, U_ONE_BUCKET, U_BUCKET_EDGE = (U_THRESH + 4 + k for k in range(4))
U_FILL = U_BUCKET_EDGE + 1
I_FILL = I_BOUND + len(LENGTHS)
N_FILL = 50
N_USERS = U_FILL + N_FILL + 1                  # the last user and the last item have no record
N_ITEMS = I_FILL + N_FILL + 1
ONE_BUCKET = 17500
EDGE_KS = (17361, 17362, 18000)                # 17361 TAU - 1 < EPOCH: the smallest timestamp


def _cols(**kw):
    from bbgr.features import ReviewColumns
    return ReviewColumns(**kw)


def _np(t):
    return t.cpu().numpy()


def _finish(rng, user, item, **fixed):
    """The other columns for (user, item): inexact ratings with ties, votes
    either side of the helpful threshold, L = 0, epoch-scale timestamps of
    which about 10 % are missing (and then hold values outside the range)."""
    E = user.size
    n_tokens = rng.integers(0, 60, E)
    n_tokens[rng.uniform(size=E) < 0.1] = 0
    n_unique = np.where(n_tokens > 0, rng.integers(0, 60, E) % np.maximum(n_tokens, 1) + 1, 0)
    ts = EPOCH + rng.integers(0, 3000 * TAU, E)
    ts_valid = rng.uniform(size=E) >= 0.1
    ts[~ts_valid] = rng.choice(np.asarray([0, 2**62]), int((~ts_valid).sum()))
    c = dict(user=user, item=item, rating=rng.choice(RATINGS, E),
             helpful_vote=rng.choice(np.asarray([0, 0, 0, 1, 5, 6, 7, 20]), E),
             verified=rng.uniform(size=E) < 0.5, timestamp=ts, n_tokens=n_tokens,
             n_unique_tokens=n_unique, ts_valid=ts_valid)
    c.update(fixed)
    return c


def _typed(c, order=None):
    order = np.arange(c["user"].size) if order is None else order
    types = dict(user=np.int32, item=np.int32, rating=np.float32, helpful_vote=np.int32,
                 verified=np.uint8, timestamp=np.int64, n_tokens=np.int32,
                 n_unique_tokens=np.int32, ts_valid=np.bool_)
    return _cols(**{k: (None if c[k] is None else np.asarray(c[k])[order].astype(t))
                    for k, t in types.items()})


def _boundary_columns():
    rng = np.random.default_rng(355)
    n_long = 513 + np.arange(N_LONG) % 7
    user = [np.repeat(np.arange(N_LONG), n_long)]                   # long users; their items
    item = [np.arange(n_long.sum()) % N_LONG]                       # dealt out: long as well
    lengths = np.asarray(LENGTHS)
    user.append(np.repeat(U_BOUND + np.arange(lengths.size), lengths))      # boundary users
    item.append(rng.integers(I_FILL, I_FILL + N_FILL, lengths.sum()))
    user.append(rng.integers(U_FILL, U_FILL + N_FILL, lengths.sum()))       # boundary items
    item.append(np.repeat(I_BOUND + np.arange(lengths.size), lengths))
    others = np.concatenate([np.arange(N_LONG), np.arange(I_FILL, I_FILL + N_FILL)])
    for u, n in ([(U_THRESH + k, 1000) for k in range(4)] +
                 [(U_NO_TS, 600), (U_FEW_TS, 600), (U_ONE_BUCKET, 513), (U_BUCKET_EDGE, 40)]):
        user.append(np.full(n, u))
        item.append(rng.choice(others, n))
    user, item = np.concatenate(user), np.concatenate(item)
    c = _finish(rng, user, item)
    for k, (h, _) in enumerate(THRESHOLDS):
        idx = np.flatnonzero(user == U_THRESH + k)
        c["helpful_vote"][idx] = 5
        c["helpful_vote"][idx[:h]] = 6
    ts, ts_valid = c["timestamp"], c["ts_valid"]
    ts_valid[user == U_NO_TS] = False
    idx = np.flatnonzero(user == U_FEW_TS)
    ts_valid[idx] = False
    ts_valid[idx[:100]] = True
    ts[idx[:100]] = EPOCH + rng.integers(0, 3000 * TAU, 100)
    idx = np.flatnonzero(user == U_ONE_BUCKET)
    ts_valid[idx] = True
    ts[idx] = ONE_BUCKET * TAU + rng.integers(0, TAU, idx.size)
    ts[idx[0]], ts[idx[1]] = ONE_BUCKET * TAU, (ONE_BUCKET + 1) * TAU - 1
    idx = np.flatnonzero(user == U_BUCKET_EDGE)
    ts_valid[idx] = True
    ts[idx] = EPOCH + rng.integers(0, 3000 * TAU, idx.size)
    for j, k in enumerate(EDGE_KS):
        ts[idx[2 * j]], ts[idx[2 * j + 1]] = k * TAU - 1, k * TAU
    return _typed(c, rng.permutation(user.size))                    # file order mixes all of it


def _build(cols, n_users, n_items):
    from bbgr.features import build_credibility_graph
    return build_credibility_graph(cols, n_users, n_items, device=DEV)


@pytest.fixture(scope="module")
def boundary():
    cols = _boundary_columns()
    return cols, FR.features_ref(cols, N_USERS, N_ITEMS), _build(cols, N_USERS, N_ITEMS)


# -- the comparison ----------------------------------------------------------------------
def _ulps(got, want):
    """Distance in float32 steps (non-negative values); the NaNs must coincide."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    d[nan] = 0
    return d


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _rows(ids, n_rows):
    """(record ids grouped by row in file order, indptr)."""
    ids = np.asarray(ids)
    counts = np.bincount(ids, minlength=n_rows)
    return np.argsort(ids, kind="stable"), np.concatenate([[0], np.cumsum(counts)])


def _fsum_means(terms, order, indptr):
    """math.fsum(terms of the row) / n per row: the sum is exact, so the mean
    carries two roundings whatever the order. NaN for an empty row."""
    return np.asarray([math.fsum(terms[order[a:b]]) / (b - a) if b > a else math.nan
                       for a, b in zip(indptr[:-1], indptr[1:])])


def _ulp32(m):
    """The float32 spacing in the binade of |m| (m in float32's normal range)."""
    return math.ldexp(1.0, math.frexp(abs(m))[1] - 24) if m else 0.0


def _mean_problems(name, got, want, m, n):
    """The two checks of a mean column; prints the largest values seen among
    the one-lane rows and among the workgroup rows, returns what fails."""
    problems = []
    d = _ulps(got, want)
    has = n > 0
    if (_bits(got[~has]) != _bits(want[~has])).any():
        problems.append(f"{name}: a row without records differs from the reference")
    bound = np.asarray([_ulp32(x) / 2 + (k + 2) * 2.0 ** -53 * abs(x)
                        for x, k in zip(m[has], n[has])])
    err = np.abs(got[has].astype(np.float64) - m[has])
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    ratio[(bound == 0) & (err > 0)] = math.inf
    for cls, sel in (("one lane", n[has] <= LONG_ROW), ("workgroup", n[has] > LONG_ROW)):
        if sel.any():
            print(f"{name}, {cls} rows ({int(sel.sum())}): largest ulp distance "
                  f"{int(d[has][sel].max())}, largest |got - m| / bound {ratio[sel].max():.4f}")
    if d.size and d.max() > 1:
        problems.append(f"{name}: {int(d.max())} ulp from the reference")
    if (err > bound).any():
        problems.append(f"{name}: {int((err > bound).sum())} rows beyond the bound, worst "
                        f"{ratio.max():.3f} of it")
    return problems


def _check(out, cols, n_users, n_items, ref=None):
    """Every output against the reference as the module docstring says; the
    order-dependent figures are printed before anything is asserted."""
    ref = FR.features_ref(cols, n_users, n_items) if ref is None else ref
    E = len(cols)
    user, item = np.asarray(cols.user), np.asarray(cols.item)
    r64 = np.asarray(cols.rating, np.float32).astype(np.float64)
    ix, ux, ea = _np(out.item_x), _np(out.user_x), _np(out.edge_attr)
    assert ix.shape == (n_items, 2) and ux.shape == (n_users, 7) and ea.shape == (E, 5)
    i_order, i_ptr = _rows(item, n_items)
    u_order, u_ptr = _rows(user, n_users)
    problems = _mean_problems("item mean", ix[:, 0], ref["item_x"][:, 0],
                              _fsum_means(r64, i_order, i_ptr), np.diff(i_ptr))
    terms = FR.user_sum_terms(cols)
    for c, name in MEAN_USER_COLS.items():
        problems += _mean_problems(name, ux[:, c], ref["user_x"][:, c],
                                   _fsum_means(terms[c], u_order, u_ptr), np.diff(u_ptr))
    d = _ulps(ux[:, 1], ref["user_x"][:, 1])
    n_u = np.diff(u_ptr)
    for cls, sel in (("one lane", (n_u > 0) & (n_u <= LONG_ROW)), ("workgroup", n_u > LONG_ROW)):
        if sel.any():
            print(f"entropy, {cls} rows: largest ulp distance {int(d[sel].max())}")
    if d.max() > 1:
        problems.append(f"entropy: {int(d.max())} ulp from the reference")

    assert out.src.dtype == torch.int32 and out.dst.dtype == torch.int32
    assert out.user_y.dtype == torch.int64 and out.total_reviews.dtype == torch.int32
    assert out.helpful_reviews.dtype == torch.int32 and out.user_y.shape == (n_users,)
    for key in ("src", "dst", "user_y", "total_reviews", "helpful_reviews"):
        np.testing.assert_array_equal(_np(getattr(out, key)), ref[key], err_msg=key)
    assert out.stats == ref["stats"]
    np.testing.assert_array_equal(ix[:, 1], ref["item_x"][:, 1])
    np.testing.assert_array_equal(ux[:, EXACT_USER_COLS], ref["user_x"][:, EXACT_USER_COLS])
    for c in (0, 2, 3, 4):
        np.testing.assert_array_equal(_bits(ea[:, c]), _bits(ref["edge_attr"][:, c]),
                                      err_msg=f"edge_attr column {c}")
    # rating_align from the device's own float32 mean: what the kernel evaluates
    align = (1.0 - np.abs(r64 - ix[item, 0].astype(np.float64)) / 4.0).astype(np.float32)
    np.testing.assert_array_equal(_bits(ea[:, 1]), _bits(align), err_msg="rating_align")
    assert not problems, problems


# -- 1. the boundary graph -----------------------------------------------------------------
def test_boundary_graph_is_what_the_issue_lists(boundary):
    cols, ref, _ = boundary
    deg_u = np.bincount(cols.user, minlength=N_USERS)
    deg_i = np.bincount(cols.item, minlength=N_ITEMS)
    np.testing.assert_array_equal(deg_u[:N_LONG], 513 + np.arange(N_LONG) % 7)
    assert (deg_i[:N_LONG] > LONG_ROW).all() and deg_i[:N_LONG].max() < 600
    # more long rows than workgroups: the long kernels' loop makes a second trip
    assert (deg_u > LONG_ROW).sum() > LONG_GRID and (deg_i > LONG_ROW).sum() > LONG_GRID
    np.testing.assert_array_equal(deg_u[U_BOUND:U_BOUND + len(LENGTHS)], LENGTHS)
    np.testing.assert_array_equal(deg_i[I_BOUND:I_BOUND + len(LENGTHS)], LENGTHS)
    assert set(LENGTHS) <= set(deg_u.tolist()) and set(LENGTHS) <= set(deg_i.tolist())
    assert deg_u[-1] == 0 and deg_i[-1] == 0
    for k, (h, label) in enumerate(THRESHOLDS):
        u = U_THRESH + k
        assert deg_u[u] == 1000 and ref["helpful_reviews"][u] == h and ref["user_y"][u] == label
    dated = np.asarray(cols.ts_valid)
    assert deg_u[U_NO_TS] == 600 and not dated[cols.user == U_NO_TS].any()
    assert deg_u[U_FEW_TS] == 600 and dated[cols.user == U_FEW_TS].sum() == 100    # < 256
    assert deg_u[U_ONE_BUCKET] == 513 and ref["user_x64"][U_ONE_BUCKET, 4] == 512
    assert ref["user_x64"][U_NO_TS, 4] == 0
    stamps = set(cols.timestamp[cols.user == U_BUCKET_EDGE].tolist())
    assert all({k * TAU - 1, k * TAU} <= stamps for k in EDGE_KS)
    assert ref["stats"]["ts_min"] == EDGE_KS[0] * TAU - 1 > 1.49e12
    assert 2999 * TAU < ref["stats"]["ts_max"] - ref["stats"]["ts_min"] < 3001 * TAU
    assert 0.08 < 1 - dated.mean() < 0.12 and cols.timestamp[~dated].max() == 2**62
    assert set(np.unique(cols.rating).tolist()) == set(RATINGS.tolist())
    assert 160_000 < len(cols) < 200_000


def test_boundary_graph(boundary):
    cols, ref, out = boundary
    _check(out, cols, N_USERS, N_ITEMS, ref)
    assert np.isnan(_np(out.user_x[-1])).all() and int(out.user_y[-1]) == -1
    np.testing.assert_array_equal(_np(out.item_x[-1]), [0, 0])
    ts_norm = _np(out.edge_attr[:, 3])
    np.testing.assert_array_equal(np.isnan(ts_norm), ~np.asarray(cols.ts_valid))
    assert np.nanmin(ts_norm) == 0 and np.nanmax(ts_norm) == 1


def test_boundary_graph_twice_gives_the_same_bits(boundary):
    cols, _, out = boundary
    again = _build(cols, N_USERS, N_ITEMS)
    for key in OUTPUT_KEYS:
        a, b = _np(getattr(out, key)), _np(getattr(again, key))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert out.stats == again.stats


# -- 2. the launch gate --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_row_512", "one_row_513", "one_user_513_items",
                                  "one_item_513_users"])
def test_launch_gate_and_tiny_long_cases(case):
    """The long kernels are launched for E > 512 only: E = 512 in one row is
    the longest one-lane row, E = 513 the shortest workgroup row and the only
    entry of the long-row list."""
    rng = np.random.default_rng(len(case))
    E = 512 if case == "one_row_512" else 513
    spread = rng.permutation(E)
    if case.startswith("one_row"):
        n_users, n_items, user, item = 3, 3, np.full(E, 1), np.full(E, 1)
    elif case == "one_user_513_items":
        n_users, n_items, user, item = 2, E + 1, np.full(E, 1), spread
    else:
        n_users, n_items, user, item = E + 1, 2, spread, np.full(E, 1)
    cols = _typed(_finish(rng, user, item))
    _check(_build(cols, n_users, n_items), cols, n_users, n_items)


# -- 3. tile tails of the edge kernel, and memory behind every output ----------------------
POISON32 = 0x7FC12345            # as float32: a NaN, and not the one a computation gives
POISON64 = 0x7FC123457FC12345
PAD = 96                         # elements behind the end
TILE_E = [2, 3, 255, 256, 257, 510, 511, 512, 513, 1279, 1280, 1281]


def _poisoned(shape, dtype):
    """(buffer, leading view of `shape`): PAD poisoned elements follow the view."""
    n = math.prod(shape)
    wide = dtype == torch.int64
    raw = torch.full((n + PAD,), POISON64 if wide else POISON32,
                     dtype=torch.int64 if wide else torch.int32, device=DEV)
    view = raw[:n].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0
    return raw, view


def _tail_intact(raw, n):
    want = POISON64 if raw.dtype == torch.int64 else POISON32
    return raw.numel() == n + PAD and bool((raw[n:] == want).all())


def _workspace_tail_intact(fn, *args):
    """Call `fn` with a workspace larger than its query asks for; the bytes
    behind the queried size must stay as they were."""
    from bbgr import _lib
    st = _lib.stream_handle()
    nb = _lib.workspace_query(fn, *args, args_after=(st,))
    ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.call(fn, *args, _lib.ptr(ws), ctypes.byref(ctypes.c_size_t(nb + 4096)), st)
    torch.cuda.synchronize()
    return bool((ws[nb:] == 0xA5).all())


@pytest.mark.parametrize("E", TILE_E)
def test_tile_tails_and_untouched_tails(E):
    """5 E mod 4 takes every value over TILE_E, and the last workgroup is full,
    one record short and one over; half of the records lie in one row."""
    from bbgr import _lib
    from bbgr import features as F
    n_users, n_items = 9, 5
    rng = np.random.default_rng(E)
    user = np.where(rng.uniform(size=E) < 0.5, 0, rng.integers(0, n_users - 1, E))
    item = np.where(rng.uniform(size=E) < 0.5, 0, rng.integers(0, n_items - 1, E))
    cols = _typed(_finish(rng, user, item))
    p = F._Pipeline(cols, n_users, n_items, E, torch.device("cuda", torch.cuda.current_device()))
    raws = {}
    for name, shape in (("edge_attr", (E, 5)), ("item_x", (n_items, 2)), ("user_x", (n_users, 7)),
                        ("user_y", (n_users,)), ("total", (n_users,)),
                        ("helpful_reviews", (n_users,))):
        raws[name], view = _poisoned(shape, getattr(p, name).dtype)
        assert view.shape == getattr(p, name).shape
        setattr(p, name, view)
    out = p.run()
    assert out.edge_attr.data_ptr() == raws["edge_attr"].data_ptr()
    _check(out, cols, n_users, n_items)
    for name, raw in raws.items():
        assert _tail_intact(raw, getattr(p, name).numel()), name
    # the two row passes again, each with a workspace larger than it asks for
    before = {name: raw.clone() for name, raw in raws.items()}
    assert _workspace_tail_intact("bbgr_feat_items", p.cref, _lib.ptr(p.i_indptr),
                                  _lib.ptr(p.i_eid), _lib.ptr(p.item_x), _lib.ptr(p.item_rbar))
    a = _lib.FeatUserArgs()
    a.u_indptr, a.u_eid = _lib.ptr(p.u_indptr), _lib.ptr(p.u_eid)
    a.b_indptr, a.b_bucket = _lib.ptr(p.b_indptr), _lib.ptr(p.b_bucket)
    a.item_rbar, a.global_avg_len = _lib.ptr(p.item_rbar), p.global_avg_len
    a.user_x, a.user_y = _lib.ptr(p.user_x), _lib.ptr(p.user_y)
    a.total_reviews, a.helpful_reviews = _lib.ptr(p.total), _lib.ptr(p.helpful_reviews)
    assert _workspace_tail_intact("bbgr_feat_users", p.cref, ctypes.byref(a))
    for name, raw in raws.items():
        assert torch.equal(raw, before[name]), name


# -- 4. statistics beyond one grid pass ----------------------------------------------------
@pytest.mark.parametrize("mask", ["some", "all_false", "none"])
def test_stats_beyond_one_grid_pass(mask):
    """E = 262144 + 300: the records from 262144 on are reached by the strided
    second trip only, and both extremes of the valid timestamps lie there."""
    from bbgr import features as F
    E = STATS_THREADS + 300
    rng = np.random.default_rng(4)
    ts = EPOCH + rng.integers(1000 * TAU, 2000 * TAU, E)
    valid = rng.uniform(size=E) >= 0.1
    ts[E - 1], valid[E - 1] = -7 * TAU - 3, True                    # the smallest valid
    ts[STATS_THREADS], valid[STATS_THREADS] = EPOCH + 2500 * TAU, True      # the largest
    ts[5], valid[5] = -3, True                                      # negative, not the smallest
    for e in (100, STATS_THREADS + 50):                             # smaller still, not valid
        ts[e], valid[e] = -9 * TAU, False
    ts[STATS_THREADS + 60], valid[STATS_THREADS + 60] = EPOCH + 2900 * TAU, False
    n_tokens = rng.integers(0, 60, E)
    n_tokens[[7, 4096, STATS_THREADS - 1, STATS_THREADS + 7, E - 2]] = 2**31 - 1
    assert int(n_tokens.sum()) > 2**32
    valid = {"some": valid, "all_false": np.zeros(E, bool), "none": None}[mask]
    zeros = np.zeros(E, np.int32)
    cols = _typed(dict(user=zeros, item=zeros, rating=zeros, helpful_vote=zeros, verified=zeros,
                       timestamp=ts, n_tokens=n_tokens, n_unique_tokens=zeros, ts_valid=valid))
    p = F._Pipeline(cols, 1, 1, E, torch.device("cuda", torch.cuda.current_device()))
    p.stats()
    p.read_stats()
    seen = ts[valid] if valid is not None else ts
    assert p.n_ts == seen.size
    if seen.size:
        assert (p.ts_min, p.ts_max) == (int(seen.min()), int(seen.max()))
    else:
        assert (p.ts_min, p.ts_max) == (2**63 - 1, -2**63)
    if mask == "some":
        assert (p.ts_min, p.ts_max) == (-7 * TAU - 3, EPOCH + 2500 * TAU)
    if mask == "none":
        assert (p.ts_min, p.ts_max) == (-9 * TAU, EPOCH + 2900 * TAU)
    assert _np(p.stats_dev)[3] == n_tokens.sum(dtype=np.int64)
    assert p.global_avg_len == int(n_tokens.sum(dtype=np.int64)) / E


# -- 5. bbgr_csr_build as the features call it ---------------------------------------------
def _i32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).to(DEV)


def _indptr_ref(rows, n_rows):
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))])


@pytest.mark.parametrize("ids", ["seven_values", "all_equal"])
@pytest.mark.parametrize("E", [1, 255, 256, 257, 4097, 100003])
def test_group_by_the_id_alone(E, ids):
    """n_cols = 1 over a column of zeros: the stable sort's permutation lists
    every row's records in file order."""
    from bbgr import features as F
    n_rows = 13                                                     # rows 0..2 and 10..12 empty
    rng = np.random.default_rng(E)
    rows = rng.integers(3, 10, E) if ids == "seven_values" else np.full(E, 6)
    indptr, eid = F._group(_i32(rows), torch.zeros(E, dtype=torch.int32, device=DEV), n_rows)
    assert indptr.dtype == torch.int32 and eid.dtype == torch.int32
    np.testing.assert_array_equal(_np(eid)[:E], np.argsort(rows, kind="stable"))
    np.testing.assert_array_equal(_np(indptr), _indptr_ref(rows, n_rows))
    assert (_np(indptr)[:4] == 0).all() and (_np(indptr)[10:] == E).all()


def _csr_against_lexsort(rows, cols, n_rows, n_cols):
    from bbgr import features as F
    E = rows.size
    perm = torch.empty(E, dtype=torch.int32, device=DEV)
    indptr, indices = F._csr_build(_i32(rows), _i32(cols), n_rows, n_cols, perm=perm)
    order = np.lexsort((np.arange(E), cols, rows))
    np.testing.assert_array_equal(_np(perm), order)                 # equal pairs ascend
    np.testing.assert_array_equal(_np(indices)[:E], cols[order])
    np.testing.assert_array_equal(_np(indptr), _indptr_ref(rows, n_rows))
    np.testing.assert_array_equal(_np(indptr),
                                  np.searchsorted(rows[order], np.arange(n_rows + 1)))


@pytest.mark.parametrize("n_rows,n_cols", [(70001, 2**31 - 1), (2**16, 2**15)])
def test_csr_build_wide_keys(n_rows, n_cols):
    """Keys beyond 2^47 (the radix sort's end bit comes from n_rows n_cols), and
    a key range that is an exact power of two with its largest key present."""
    rng = np.random.default_rng(n_rows)
    rows = np.concatenate([rng.integers(0, n_rows, 4500), [0, 0, n_rows - 1, n_rows - 1]])
    cols = np.concatenate([rng.integers(0, n_cols, 4500), [0, n_cols - 1, 0, n_cols - 1]])
    again = rng.integers(0, rows.size, 500)                         # duplicate pairs
    rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
    order = rng.permutation(rows.size)
    rows, cols = rows[order], cols[order]
    keys = rows.astype(np.int64) * n_cols + cols
    assert keys.max() == n_rows * n_cols - 1 and np.unique(keys).size < keys.size
    if n_cols == 2**31 - 1:
        assert keys.max() > 2**47
    else:
        assert n_rows * n_cols == 2**31
    _csr_against_lexsort(rows, cols, n_rows, n_cols)


def test_csr_build_bucket_shape():
    """The bucket build: n_rows = U + 1, the spare row U full of (U, 0) pairs."""
    n_users, n_cols, E = 500, 3001, 20000
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, n_users, E), rng.integers(0, n_cols, E)
    spare = rng.uniform(size=E) < 0.1
    rows[spare], cols[spare] = n_users, 0
    rows[:50], cols[:50] = 7, 3000                                  # a run of equal pairs
    assert spare.sum() > 1500
    _csr_against_lexsort(rows, cols, n_users + 1, n_cols)
