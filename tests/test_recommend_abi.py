"""CPU: bbgr_recommend / bbgr_eval_lists argument validation and workspace
queries through ctypes (host code only: every check runs before any launch)."""
import ctypes

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced


def _args(**kw):
    a = _lib.RecommendArgs()
    a.n_users, a.n_user_rows, a.n_items, a.d, a.k = 1000, 5000, 3000, 64, 20
    a.lduf = a.ldif = 64
    a.users = a.uf = a.itf = a.topk = FAKE
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _rc(a, ws=None, nbytes=0):
    n = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_recommend(ctypes.byref(a), ws, ctypes.byref(n), None)
    return rc, _lib.lib().bbgr_last_error().decode(), n.value


def test_abi_version_is_still_12():
    assert _lib.lib().bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    import subprocess
    src = ('#include "bbgr.h"\n#include <stdio.h>\n'
           'int main(){printf("%zu", sizeof(bbgr_recommend_args));}')
    exe = str(tmp_path / "sizeof_recommend_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(_lib.RecommendArgs)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("k", [1, 16, 17, 128])
def test_workspace_query_is_positive(d, k):
    rc, _, n = _rc(_args(d=d, k=k, lduf=d, ldif=d))
    assert rc == 0 and n > 0
    # at least one list pair per lane half and user, and the per-user bound
    assert n >= 1000 * 2 * 16 * 8 + 1000 * 8


def test_workspace_query_with_exclusion_and_mask():
    rc, _, n = _rc(_args(ex_indptr=FAKE, ex_indices=FAKE, item_mask=FAKE, topk_score=FAKE))
    assert rc == 0 and n > 0


def test_no_users_is_ok_without_a_launch():
    a = _args(n_users=0, users=None, topk=None)
    rc, _, n = _rc(a)
    assert rc == 0
    buf = ctypes.create_string_buffer(max(n, 1))
    rc, msg, _ = _rc(a, buf, max(n, 1))
    assert rc == 0, msg


@pytest.mark.parametrize("kw,field", [
    (dict(users=None), "users"),
    (dict(uf=None), "uf"),
    (dict(itf=None), "itf"),
    (dict(topk=None), "topk"),
    (dict(k=0), "k"),
    (dict(k=129), "k"),
    (dict(n_items=0), "n_items"),
    (dict(n_items=-5), "n_items"),
    (dict(n_users=-1), "n_users"),
    (dict(n_user_rows=0), "n_user_rows"),
    (dict(uf=FAKE + 4), "uf"),
    (dict(itf=FAKE + 8), "itf"),
    (dict(lduf=66), "lduf"),
    (dict(ldif=65), "ldif"),
    (dict(ex_indptr=FAKE), "ex_indices"),
    (dict(ex_indices=FAKE), "ex_indptr"),
])
def test_invalid_arguments_name_the_field(kw, field):
    rc, msg, _ = _rc(_args(**kw))
    assert rc == -1, msg
    assert msg.startswith("bbgr_recommend:") and field in msg, msg


def test_null_args_and_null_size():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.bbgr_recommend(None, None, ctypes.byref(n), None) == -1
    assert b"null args" in L.bbgr_last_error()
    a = _args()
    assert L.bbgr_recommend(ctypes.byref(a), None, None, None) == -1
    assert b"workspace_bytes" in L.bbgr_last_error()


@pytest.mark.parametrize("d", [8, 32, 48, 96, 512, 0])
def test_unsupported_width(d):
    rc, msg, _ = _rc(_args(d=d))
    assert rc == -2 and str(d) in msg and "unsupported" in msg


def test_small_workspace_is_refused_before_any_launch():
    a = _args()
    _, _, n = _rc(a)
    rc, msg, _ = _rc(a, ctypes.c_void_p(FAKE), n - 1)
    assert rc == -4 and "workspace" in msg


def _eval_args():
    a = _lib.EvalArgs()
    a.n_users, a.n_items, a.k_max, a.n_k = 10000, 5000, 128, 2
    a.ks[0], a.ks[1] = 50, 100
    a.users = a.te_indptr = a.te_indices = a.topk = a.item_pop = a.sums = FAKE
    return a


def test_eval_lists_workspace_query_and_limits():
    """uf / itf / d and the train CSR are ignored (left null here)."""
    a = _eval_args()
    n = ctypes.c_size_t(0)
    _lib.call("bbgr_eval_lists", ctypes.byref(a), None, ctypes.byref(n), None)
    assert n.value >= 2 * 5000 + 8 * 2 * 3 * 10
    a.k_max = 129
    with pytest.raises(_lib.BbgrError, match="k_max <= 128"):
        _lib.call("bbgr_eval_lists", ctypes.byref(a), None, ctypes.byref(n), None)
    a.k_max, a.topk = 128, None
    with pytest.raises(_lib.BbgrError, match="BBGR_ERR_INVALID.*topk"):
        _lib.call("bbgr_eval_lists", ctypes.byref(a), None, ctypes.byref(n), None)
    a.topk, a.ks[1] = FAKE, 129
    with pytest.raises(_lib.BbgrError, match=r"ks\[1\]"):
        _lib.call("bbgr_eval_lists", ctypes.byref(a), None, ctypes.byref(n), None)
    a.ks[1] = 100
    with pytest.raises(_lib.BbgrError, match="BBGR_ERR_WORKSPACE"):
        small = ctypes.c_size_t(8)
        _lib.call("bbgr_eval_lists", ctypes.byref(a), ctypes.c_void_p(FAKE), ctypes.byref(small),
                  None)
