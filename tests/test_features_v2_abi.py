"""CPU: bbgr_text_unique_pooled, bbgr_feat_gaps and bbgr_feat_users_v2 (and
the two small passes beside them) through ctypes: the symbols resolve, the
struct layout agrees with the header, the size queries answer, every argument
error is BBGR_ERR_INVALID naming the argument before any launch, and the
Python entry points refuse what they must before they touch the GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
SYMBOLS = ["bbgr_text_unique_pooled", "bbgr_feat_gaps", "bbgr_feat_users_v2"]
BESIDE = ["bbgr_text_unique_pooled_stages", "bbgr_feat_lenlog", "bbgr_feat_item_means"]


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbols_resolve_and_abi_is_still_12():
    L = _lib.lib()
    for s in SYMBOLS + BESIDE:
        assert hasattr(L, s) and s in _lib._SIGNATURES and s in _lib.header_symbols(), s
    assert L.bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    names = [f[0] for f in _lib.FeatUserV2Args._fields_]
    assert names == ["u_indptr", "u_eid", "b_indptr", "b_bucket", "item_mean",
                     "global_avg_lenlog", "group_tokens", "group_unique", "etg", "user_x",
                     "user_y", "total_reviews", "helpful_reviews", "user_extra"]
    prints = "".join(f'printf(" %zu", offsetof(bbgr_feat_user_v2_args, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof(bbgr_feat_user_v2_args));{prints}}}')
    exe = str(tmp_path / "layout_user_v2_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.FeatUserV2Args)
    assert [int(v) for v in out[1:]] == [getattr(_lib.FeatUserV2Args, f).offset for f in names]


# -- bbgr_text_unique_pooled ---------------------------------------------------------------
def _text(**kw):
    a = _lib.TextArgs()
    a.n, a.first, a.last, a.hash_mask = 1000, 0, 350_000, 0
    a.data = a.offsets = a.n_tokens = a.n_unique_tokens = a.recheck = a.totals = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pooled(a, total=60_000, group=FAKE, n_groups=50, tokens=FAKE, unique=FAKE, flag=FAKE,
            ws=FAKE, nbytes=1 << 40):
    n = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_text_unique_pooled(None if a is None else ctypes.byref(a), total, group,
                                            n_groups, tokens, unique, flag, ws, ctypes.byref(n),
                                            None)
    return rc, n.value


def test_pooled_size_query():
    rc, nb = _pooled(_text(), ws=None, nbytes=0)
    assert rc == 0, _err()
    # the per-record stream's workspace, and 8 bytes per token more for the group keys
    n = ctypes.c_size_t(0)
    a = _text()
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), 60_000, None, ctypes.byref(n), None) == 0
    assert nb >= n.value + 8 * 60_000
    rc, _ = _pooled(_text(), nbytes=nb - 1)
    assert rc == -4 and "workspace" in _err(), _err()
    rc, nb0 = _pooled(_text(n=0, last=0), total=0, n_groups=0, ws=None, nbytes=0)
    assert rc == 0, _err()


POOLED_BAD = [
    (dict(a=None), "null args"), (dict(n_groups=-1), "n_groups out of range"),
    (dict(total=-1), "total_tokens out of range"), (dict(total=175_501), "total_tokens out of range"),
    (dict(total=2**40), "total_tokens out of range"), (dict(group=None), "null group"),
    (dict(tokens=None), "null group_tokens"), (dict(unique=None), "null group_unique"),
    (dict(flag=None), "null group_recheck"),
]


@pytest.mark.parametrize("kw,what", POOLED_BAD)
def test_pooled_arguments_are_validated(kw, what):
    kw = dict(kw)
    a = kw.pop("a", _text())
    for ws in (FAKE, None):                   # refused in a size query too
        rc, _ = _pooled(a, ws=ws, **kw)
        assert rc == -1, _err()
        assert _err().startswith("bbgr_text_unique_pooled:") and what in _err(), _err()


@pytest.mark.parametrize("kw,what", [(dict(totals=None), "null totals"), (dict(n=-1), "n out of range"),
                                     (dict(last=2**31 - 1), "first / last out of range"),
                                     (dict(data=None), "null data"),
                                     (dict(offsets=None), "null offsets")])
def test_pooled_text_arguments_are_validated(kw, what):
    rc, _ = _pooled(_text(**kw))
    assert rc == -1 and what in _err(), _err()


def test_pooled_stages_range():
    n = ctypes.c_size_t(1 << 40)
    a = _text()
    for stages in (0, 8, -1):
        rc = _lib.lib().bbgr_text_unique_pooled_stages(ctypes.byref(a), 60_000, FAKE, 50, FAKE,
                                                       FAKE, FAKE, stages, FAKE, ctypes.byref(n),
                                                       None)
        assert rc == -1 and "stages out of range" in _err(), _err()


# -- the feature passes --------------------------------------------------------------------
def _columns(**kw):
    c = _lib.FeatColumns()
    c.n, c.n_users, c.n_items = 1000, 30, 20
    c.user = c.item = c.rating = c.helpful_vote = c.verified = c.timestamp = FAKE
    c.n_tokens = c.n_unique_tokens = FAKE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _user_args(**kw):
    a = _lib.FeatUserV2Args()
    for name, _ in _lib.FeatUserV2Args._fields_:
        setattr(a, name, 0.5 if name == "global_avg_lenlog" else FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(fn, *args, ws=FAKE, nbytes=1 << 40):
    n = ctypes.c_size_t(nbytes)
    rc = getattr(_lib.lib(), fn)(*args, ws, ctypes.byref(n), None)
    return rc, n.value


def test_feature_size_queries():
    c = ctypes.byref(_columns())
    rc, gaps = _call("bbgr_feat_gaps", c, FAKE, FAKE, FAKE, ws=None, nbytes=0)
    assert rc == 0 and gaps >= 16 * 1000, _err()             # two doubles a record, the sort's own
    rc, users = _call("bbgr_feat_users_v2", c, ctypes.byref(_user_args()), ws=None, nbytes=0)
    assert rc == 0 and users >= 16 * 1000, _err()            # the packed records
    rc, small = _call("bbgr_feat_lenlog", c, FAKE, ws=None, nbytes=0)
    assert rc == 0 and small >= 8 * 256, _err()
    rc, _ = _call("bbgr_feat_item_means", c, FAKE, FAKE, FAKE, ws=None, nbytes=0)
    assert rc == 0, _err()
    for fn, args, need in (("bbgr_feat_gaps", (c, FAKE, FAKE, FAKE), gaps),
                           ("bbgr_feat_users_v2", (c, ctypes.byref(_user_args())), users)):
        rc, _ = _call(fn, *args, nbytes=need - 1)
        assert rc == -4 and "workspace" in _err(), _err()


@pytest.mark.parametrize("cols,args,what", [
    (None, (FAKE, FAKE, FAKE), "null columns"), (dict(n=-1), (FAKE, FAKE, FAKE), "n out of range"),
    (dict(timestamp=None), (FAKE, FAKE, FAKE), "null timestamp"),
    ({}, (None, FAKE, FAKE), "null u_indptr"), ({}, (FAKE, None, FAKE), "null u_eid"),
    ({}, (FAKE, FAKE, None), "null etg")])
def test_gaps_arguments_are_validated(cols, args, what):
    c = None if cols is None else ctypes.byref(_columns(**cols))
    rc, _ = _call("bbgr_feat_gaps", c, *args)
    assert rc == -1 and _err().startswith("bbgr_feat_gaps:") and what in _err(), _err()


@pytest.mark.parametrize("field", [f for f, _ in _lib.FeatUserV2Args._fields_
                                   if f != "global_avg_lenlog"])
def test_users_v2_null_pointers_are_refused(field):
    rc, _ = _call("bbgr_feat_users_v2", ctypes.byref(_columns()),
                  ctypes.byref(_user_args(**{field: None})))
    assert rc == -1, _err()
    assert _err().startswith("bbgr_feat_users_v2:") and f"null {field}" in _err(), _err()


def test_users_v2_null_structs_are_refused():
    rc, _ = _call("bbgr_feat_users_v2", None, ctypes.byref(_user_args()))
    assert rc == -1 and "null columns" in _err()
    rc, _ = _call("bbgr_feat_users_v2", ctypes.byref(_columns()), None)
    assert rc == -1 and "null args" in _err()


# -- the Python entry points, before they touch the GPU -------------------------------------
def _cols(n=3, text=None):
    from bbgr.features import ReviewColumns
    z = np.zeros(n, np.int32)
    return ReviewColumns(user=z, item=z, rating=np.ones(n, np.float32), helpful_vote=z,
                         verified=z.astype(np.uint8), timestamp=z.astype(np.int64), n_tokens=z,
                         n_unique_tokens=z, text=text)


def test_v2_needs_text():
    from bbgr.features import USER_EXTRA_KEYS, build_credibility_graph
    assert USER_EXTRA_KEYS == ["RNR", "ETG"]
    with pytest.raises(ValueError, match="text"):
        build_credibility_graph(_cols(), 1, 1, feature_set="v2")


def test_unknown_feature_set():
    from bbgr.features import build_credibility_graph
    with pytest.raises(ValueError, match="feature_set"):
        build_credibility_graph(_cols(), 1, 1, feature_set="v3")


def test_text_of_one_chunk_only():
    """2^31 - 1 bytes or more, faked through the offsets: refused by its size,
    with the limit named, before the bytes are looked at."""
    from bbgr.features import build_credibility_graph
    from bbgr.text import ReviewText, pooled_token_counts
    text = ReviewText(np.zeros(8, np.uint8), np.asarray([0, 5, 7, 2**31 - 1], np.int64))
    with pytest.raises(ValueError, match=r"2\^31 - 1 bytes"):
        build_credibility_graph(_cols(3, text), 1, 1, feature_set="v2")
    with pytest.raises(ValueError, match=r"2\^31 - 1 bytes"):
        pooled_token_counts(text, np.zeros(3, np.int32), 1)
