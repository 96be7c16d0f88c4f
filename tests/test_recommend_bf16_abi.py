"""CPU: bbgr_recommend_bf16 / bbgr_row_norm_max / bbgr_recommend_rescore
argument validation and workspace queries through ctypes (host code only: every
check runs before any launch). Mirrors tests/test_recommend_abi.py."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced


def _args(**kw):
    a = _lib.RecommendBf16Args()
    a.n_users, a.n_user_rows, a.n_items, a.d, a.k = 1000, 5000, 3000, 64, 20
    a.lduf = a.ldif = 64
    a.users = a.uf = a.itf = a.topk = FAKE
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _rc(a, ws=None, nbytes=0):
    n = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_recommend_bf16(ctypes.byref(a), ws, ctypes.byref(n), None)
    return rc, _lib.lib().bbgr_last_error().decode(), n.value


def _rescore(**kw):
    a = _lib.RecommendRescoreArgs()
    a.n_users, a.n_user_rows, a.n_items, a.d, a.k, a.k_pre = 1000, 5000, 3000, 64, 20, 40
    a.lduf = a.ldif = 64
    a.users = a.uf = a.itf = a.cand = a.cand_score = a.n_max = a.topk = a.certified = FAKE
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _rrc(a):
    rc = _lib.lib().bbgr_recommend_rescore(ctypes.byref(a), None)
    return rc, _lib.lib().bbgr_last_error().decode()


def test_abi_version_is_still_12():
    assert _lib.lib().bbgr_abi_version() == 12


@pytest.mark.parametrize("cname,pyty", [("bbgr_recommend_bf16_args", _lib.RecommendBf16Args),
                                        ("bbgr_recommend_rescore_args",
                                         _lib.RecommendRescoreArgs)])
def test_struct_layout_matches_header(cname, pyty, tmp_path):
    """Size and the offset of every field."""
    fields = [f[0] for f in pyty._fields_]
    body = "".join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields)
    src = ('#include "bbgr.h"\n#include <stddef.h>\n#include <stdio.h>\n'
           f'int main(){{printf("%zu", sizeof({cname}));{body}}}')
    exe = str(tmp_path / ("layout_" + cname))
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = [int(x) for x in
           subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(pyty)
    assert out[1:] == [getattr(pyty, f).offset for f in fields]


def test_bf16_args_have_the_fp32_layout():
    assert ctypes.sizeof(_lib.RecommendBf16Args) == ctypes.sizeof(_lib.RecommendArgs)


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
    rc, msg = _rrc(_rescore(n_users=0, users=None, topk=None, cand=None, certified=None))
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
    (dict(uf=FAKE + 8), "uf"),
    (dict(itf=FAKE + 8), "itf"),
    (dict(lduf=68), "lduf"),          # a multiple of 4, not of 8
    (dict(ldif=65), "ldif"),
    (dict(ldif=76), "ldif"),
    (dict(lduf=56), "lduf"),          # < d
    (dict(ex_indptr=FAKE), "ex_indices"),
    (dict(ex_indices=FAKE), "ex_indptr"),
])
def test_invalid_arguments_name_the_field(kw, field):
    rc, msg, _ = _rc(_args(**kw))
    assert rc == -1, msg
    assert msg.startswith("bbgr_recommend_bf16:") and field in msg, msg


def test_null_args_and_null_size():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.bbgr_recommend_bf16(None, None, ctypes.byref(n), None) == -1
    assert b"null args" in L.bbgr_last_error()
    a = _args()
    assert L.bbgr_recommend_bf16(ctypes.byref(a), None, None, None) == -1
    assert b"workspace_bytes" in L.bbgr_last_error()
    assert L.bbgr_recommend_rescore(None, None) == -1
    assert b"null args" in L.bbgr_last_error()


@pytest.mark.parametrize("d", [48, 4, 512, 8, 32, 0])
def test_unsupported_width(d):
    rc, msg, _ = _rc(_args(d=d))
    assert rc == -2 and str(d) in msg and "unsupported" in msg
    rc, msg = _rrc(_rescore(d=d))
    assert rc == -2 and str(d) in msg and "unsupported" in msg


def test_small_workspace_is_refused_before_any_launch():
    a = _args()
    _, _, n = _rc(a)
    rc, msg, _ = _rc(a, ctypes.c_void_p(FAKE), n - 1)
    assert rc == -4 and "workspace" in msg


@pytest.mark.parametrize("kw,field", [
    (dict(users=None), "users"),
    (dict(uf=None), "uf"),
    (dict(itf=None), "itf"),
    (dict(cand=None), "cand"),
    (dict(cand_score=None), "cand_score"),
    (dict(n_max=None), "n_max"),
    (dict(topk=None), "topk"),
    (dict(certified=None), "certified"),
    (dict(k=0), "k"),
    (dict(k=129, k_pre=129), "k"),
    (dict(k=41), "k_pre"),            # k_pre < k
    (dict(k_pre=19), "k_pre"),
    (dict(k_pre=129), "k_pre"),       # k_pre > 128
    (dict(n_items=0), "n_items"),
    (dict(n_users=-1), "n_users"),
    (dict(n_user_rows=0), "n_user_rows"),
    (dict(uf=FAKE + 4), "uf"),
    (dict(itf=FAKE + 8), "itf"),
    (dict(lduf=66), "lduf"),
    (dict(ldif=60), "ldif"),
])
def test_rescore_invalid_arguments_name_the_field(kw, field):
    rc, msg = _rrc(_rescore(**kw))
    assert rc == -1, msg
    assert msg.startswith("bbgr_recommend_rescore:") and field in msg, msg


@pytest.mark.parametrize("args,field", [
    ((-1, 64, FAKE, 64, FAKE), "n_rows"),
    ((10, 0, FAKE, 64, FAKE), "d"),
    ((10, 66, FAKE, 68, FAKE), "d"),
    ((10, 260, FAKE, 260, FAKE), "d"),
    ((10, 64, FAKE, 64, None), "out"),
    ((10, 64, None, 64, FAKE), "src"),
    ((10, 64, FAKE + 4, 64, FAKE), "src"),
    ((10, 64, FAKE, 60, FAKE), "ld"),
    ((10, 64, FAKE, 66, FAKE), "ld"),
])
def test_row_norm_max_validates(args, field):
    L = _lib.lib()
    assert L.bbgr_row_norm_max(*args, None) == -1
    msg = L.bbgr_last_error().decode()
    assert msg.startswith("bbgr_row_norm_max:") and field in msg, msg
