"""CPU: the bbgr_feat_* entry points through ctypes: the symbols resolve, the
struct layouts agree with the header, arguments are validated and workspaces
sized on the host (every check runs before any launch), and the ABI is still 12."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
SYMBOLS = ["bbgr_feat_stats", "bbgr_feat_buckets", "bbgr_feat_items", "bbgr_feat_users",
           "bbgr_feat_edges"]
TAU = 86_400_000


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbols_resolve_and_abi_is_still_12():
    L = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGNATURES and s in _lib.header_symbols(), s
    assert L.bbgr_abi_version() == 12


@pytest.mark.parametrize("cname,pyty", [("bbgr_feat_columns", _lib.FeatColumns),
                                        ("bbgr_feat_user_args", _lib.FeatUserArgs)])
def test_struct_layout_matches_header(cname, pyty, tmp_path):
    """sizeof and every field's offset (a swap of two same-sized fields keeps the size)."""
    names = [f[0] for f in pyty._fields_]
    prints = "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof({cname}));{prints}}}')
    exe = str(tmp_path / ("layout_" + cname))
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(pyty)
    assert [int(v) for v in out[1:]] == [getattr(pyty, f).offset for f in names]


def _columns(**kw):
    c = _lib.FeatColumns()
    c.n, c.n_users, c.n_items = 1000, 50, 40
    c.user = c.item = c.rating = c.helpful_vote = c.verified = c.timestamp = FAKE
    c.n_tokens = c.n_unique_tokens = FAKE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _user_args(**kw):
    a = _lib.FeatUserArgs()
    a.u_indptr = a.u_eid = a.b_indptr = a.b_bucket = a.item_rbar = FAKE
    a.user_x = a.user_y = a.total_reviews = a.helpful_reviews = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(name, c, ws=FAKE, nbytes=1 << 30):
    L = _lib.lib()
    n = ctypes.c_size_t(nbytes)
    if name == "bbgr_feat_stats":
        return L.bbgr_feat_stats(c, FAKE, None)
    if name == "bbgr_feat_buckets":
        return L.bbgr_feat_buckets(c, 0, TAU, FAKE, FAKE, ctypes.byref(ctypes.c_int32()), None)
    if name == "bbgr_feat_items":
        return L.bbgr_feat_items(c, FAKE, FAKE, FAKE, FAKE, ws, ctypes.byref(n), None)
    if name == "bbgr_feat_users":
        return L.bbgr_feat_users(c, ctypes.byref(_user_args()), ws, ctypes.byref(n), None)
    return L.bbgr_feat_edges(c, FAKE, 0, TAU, FAKE, None)


@pytest.mark.parametrize("name", SYMBOLS)
@pytest.mark.parametrize("kw,field", [
    (dict(user=None), "user"), (dict(item=None), "item"), (dict(rating=None), "rating"),
    (dict(helpful_vote=None), "helpful_vote"), (dict(verified=None), "verified"),
    (dict(timestamp=None), "timestamp"), (dict(n_tokens=None), "n_tokens"),
    (dict(n_unique_tokens=None), "n_unique_tokens"), (dict(n=-1), "n out of range"),
    (dict(n=2**31 - 1), "n out of range"), (dict(n_users=-1), "n_users"),
    (dict(n_users=2**31 - 1), "n_users"), (dict(n_items=-1), "n_items"),
    (dict(n_users=0), "n_users"),
])
def test_columns_are_validated_by_every_entry_point(name, kw, field):
    rc = _call(name, ctypes.byref(_columns(**kw)))
    assert rc == -1, _err()
    assert _err().startswith(name + ":") and field in _err(), _err()


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_columns(name):
    assert _call(name, None) == -1 and "null columns" in _err()


def test_bucket_range_must_fit_int32():
    """2^31 - 1 buckets between ts_min and ts_max would need 2^31 columns."""
    L = _lib.lib()
    n_cols = ctypes.c_int32(-7)
    c = ctypes.byref(_columns())
    rc = L.bbgr_feat_buckets(c, -TAU, (2**31 - 2) * TAU, FAKE, FAKE, ctypes.byref(n_cols), None)
    assert rc == -1 and "timestamp" in _err() and "int32" in _err(), _err()
    assert n_cols.value == -7
    rc = L.bbgr_feat_buckets(c, -2**63, 2**63 - 1, FAKE, FAKE, ctypes.byref(n_cols), None)
    assert rc == -1 and "timestamp" in _err()
    # the widest range that fits, and floor division of a negative timestamp, on an empty list
    e = ctypes.byref(_columns(n=0))
    assert L.bbgr_feat_buckets(e, -1, (2**31 - 2) * TAU - 1, None, None,
                               ctypes.byref(n_cols), None) == 0, _err()
    assert n_cols.value == 2**31 - 1
    assert L.bbgr_feat_buckets(e, -TAU - 1, TAU, None, None, ctypes.byref(n_cols), None) == 0
    assert n_cols.value == 4                                  # buckets -2 .. 1
    # no timestamp at all (ts_min > ts_max): one column
    assert L.bbgr_feat_buckets(e, 2**63 - 1, -2**63, None, None, ctypes.byref(n_cols), None) == 0
    assert n_cols.value == 1
    assert L.bbgr_feat_buckets(c, 0, TAU, FAKE, FAKE, None, None) == -1 and "n_cols" in _err()
    assert L.bbgr_feat_buckets(c, 0, TAU, None, FAKE, ctypes.byref(n_cols), None) == -1
    assert "rows" in _err()
    assert L.bbgr_feat_buckets(c, 0, TAU, FAKE, None, ctypes.byref(n_cols), None) == -1
    assert "cols" in _err()


@pytest.mark.parametrize("name", ["bbgr_feat_items", "bbgr_feat_users"])
def test_workspace_query_and_small_workspace(name):
    n = ctypes.c_size_t(0)
    c = _columns(n=1_000_000)
    L = _lib.lib()
    if name == "bbgr_feat_items":
        rc = L.bbgr_feat_items(ctypes.byref(c), FAKE, FAKE, FAKE, FAKE, None, ctypes.byref(n), None)
    else:
        rc = L.bbgr_feat_users(ctypes.byref(c), ctypes.byref(_user_args()), None, ctypes.byref(n),
                               None)
    assert rc == 0, _err()
    # the counter and one list entry per row that can be long (more than 512 records); the
    # user pass also packs 16 bytes per record
    packed = 16 * 1_000_000 if name == "bbgr_feat_users" else 0
    assert packed + 4 * (1_000_000 // 512 + 1) <= n.value <= packed + (1 << 16)
    assert _call(name, ctypes.byref(c), FAKE, n.value - 1) == -4 and "workspace" in _err()


def test_items_and_users_arguments():
    L = _lib.lib()
    c = ctypes.byref(_columns())
    n = ctypes.c_size_t(1 << 30)
    for k, args in enumerate([(None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE),
                              (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)]):
        assert L.bbgr_feat_items(c, *args, FAKE, ctypes.byref(n), None) == -1
        assert ["i_indptr", "i_eid", "item_x", "item_rbar"][k] in _err()
    assert L.bbgr_feat_items(c, FAKE, FAKE, FAKE, FAKE, FAKE, None, None) == -1
    assert "workspace_bytes" in _err()
    for field in ["u_indptr", "u_eid", "b_indptr", "b_bucket", "item_rbar", "user_x", "user_y",
                  "total_reviews", "helpful_reviews"]:
        a = _user_args(**{field: None})
        assert L.bbgr_feat_users(c, ctypes.byref(a), FAKE, ctypes.byref(n), None) == -1
        assert _err().startswith("bbgr_feat_users:") and field in _err(), _err()
    assert L.bbgr_feat_users(c, None, FAKE, ctypes.byref(n), None) == -1 and "null args" in _err()
    assert L.bbgr_feat_stats(c, None, None) == -1 and "stats" in _err()
    assert L.bbgr_feat_edges(c, None, 0, 1, FAKE, None) == -1 and "item_x" in _err()
    assert L.bbgr_feat_edges(c, FAKE, 0, 1, None, None) == -1 and "edge_attr" in _err()


def test_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: these return before any launch."""
    L = _lib.lib()
    e = ctypes.byref(_columns(n=0, n_users=0, n_items=0, user=None, item=None, rating=None))
    n = ctypes.c_size_t(1 << 20)
    assert L.bbgr_feat_edges(e, None, 0, 0, None, None) == 0
    assert L.bbgr_feat_items(e, None, None, None, None, FAKE, ctypes.byref(n), None) == 0
    assert L.bbgr_feat_users(e, ctypes.byref(_lib.FeatUserArgs()), FAKE, ctypes.byref(n), None) == 0


def test_python_checks_run_on_the_host():
    """Ids and sizes are refused before the device is touched (no GPU here)."""
    import numpy as np
    from bbgr.features import ReviewColumns, build_credibility_graph
    z = np.zeros(3, np.int32)

    def cols(**kw):
        c = ReviewColumns(z, z, z.astype(np.float32), z, z.astype(np.uint8), z.astype(np.int64),
                          z, z)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    with pytest.raises(ValueError, match=r"user id out of range: \[0, 5\].*num_users = 5"):
        build_credibility_graph(cols(user=np.asarray([0, 5, 1], np.int32)), 5, 1)
    with pytest.raises(ValueError, match="user id out of range"):
        build_credibility_graph(cols(user=np.asarray([0, -1, 1], np.int32)), 5, 1)
    with pytest.raises(ValueError, match=r"item id out of range: \[0, 7\].*num_items = 7"):
        build_credibility_graph(cols(item=np.asarray([7, 0, 1], np.int32)), 5, 7)
    with pytest.raises(ValueError, match="runs on the GPU"):
        build_credibility_graph(cols(), 1, 1, device="cpu")
