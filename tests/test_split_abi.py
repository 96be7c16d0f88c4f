"""CPU: bbgr_md5_pair_hash and bbgr_split_edges through ctypes: the symbols
resolve, the struct layout agrees with the header, every argument is validated
and the workspace sized on the host (before any launch), and the ABI is still 12."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
SYMBOLS = ["bbgr_md5_pair_hash", "bbgr_split_edges"]
THR = (3435973836, 3865470566)


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbols_resolve_and_abi_is_still_12():
    L = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGNATURES and s in _lib.header_symbols(), s
    assert L.bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    """sizeof and every field's offset (a swap of two same-sized fields keeps the size)."""
    names = [f[0] for f in _lib.SplitArgs._fields_]
    prints = "".join(f'printf(" %zu", offsetof(bbgr_split_args, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof(bbgr_split_args));{prints}}}')
    exe = str(tmp_path / "layout_split_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.SplitArgs)
    assert [int(v) for v in out[1:]] == [getattr(_lib.SplitArgs, f).offset for f in names]


# -- bbgr_md5_pair_hash -----------------------------------------------------------------
MD5_ARGS = ["n", "user", "item", "user_data", "user_offsets", "n_users", "item_data",
            "item_offsets", "n_items", "keep", "hash32"]


def _md5(**kw):
    a = dict(n=1000, user=FAKE, item=FAKE, user_data=FAKE, user_offsets=FAKE, n_users=50,
             item_data=FAKE, item_offsets=FAKE, n_items=40, keep=None, hash32=FAKE)
    a.update(kw)
    return _lib.lib().bbgr_md5_pair_hash(*(a[k] for k in MD5_ARGS), None)


@pytest.mark.parametrize("kw,what", [
    (dict(user=None), "null user"), (dict(item=None), "null item"),
    (dict(user_data=None), "user_data"), (dict(user_offsets=None), "user_offsets"),
    (dict(item_data=None), "item_data"), (dict(item_offsets=None), "item_offsets"),
    (dict(hash32=None), "hash32"), (dict(n=-1), "n out of range"),
    (dict(n=2**31 - 1), "n out of range"), (dict(n_users=-1), "n_users"),
    (dict(n_users=2**31 - 1), "n_users"), (dict(n_users=0), "n_users"),
    (dict(n_items=-1), "n_items"), (dict(n_items=2**31 - 1), "n_items"),
    (dict(n_items=0), "n_items"),
])
def test_md5_arguments_are_validated(kw, what):
    assert _md5(**kw) == -1, _err()
    assert _err().startswith("bbgr_md5_pair_hash:") and what in _err(), _err()


def test_md5_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: n = 0 returns before any launch, whatever the pointers."""
    assert _md5(n=0, user=None, item=None, user_data=None, user_offsets=None, n_users=0,
                item_data=None, item_offsets=None, n_items=0, hash32=None) == 0, _err()


# -- bbgr_split_edges -------------------------------------------------------------------
def _args(**kw):
    a = _lib.SplitArgs()
    a.n, a.n_users, a.n_items = 1000, 50, 40
    a.user = a.item = a.rating = a.hash32 = FAKE
    a.pos_threshold = 4.0
    a.thr_train, a.thr_val = THR
    a.user_map = a.item_map = a.user_src = a.item_src = a.edges = a.counts = FAKE
    a.ld_edges = 1000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _split(a, ws=FAKE, nbytes=1 << 30):
    n = ctypes.c_size_t(nbytes)
    return _lib.lib().bbgr_split_edges(ctypes.byref(a), ws, ctypes.byref(n), None)


@pytest.mark.parametrize("kw,what", [
    (dict(user=None), "null user"), (dict(item=None), "null item"),
    (dict(rating=None), "rating"), (dict(hash32=None), "hash32"),
    (dict(user_map=None), "user_map"), (dict(item_map=None), "item_map"),
    (dict(user_src=None), "user_src"), (dict(item_src=None), "item_src"),
    (dict(edges=None), "edges"), (dict(counts=None), "counts"),
    (dict(ld_edges=999), "ld_edges"), (dict(n=-1), "n out of range"),
    (dict(n=2**31 - 1, ld_edges=2**31 - 1), "n out of range"),
    (dict(n_users=-1), "n_users"), (dict(n_users=2**31 - 1), "n_users"),
    (dict(n_users=0), "n_users"), (dict(n_items=-1), "n_items"),
    (dict(n_items=2**31 - 1), "n_items"), (dict(n_items=0), "n_items"),
    (dict(thr_train=THR[1] + 1), "thr_train > thr_val"),
    (dict(thr_val=2**32 + 1), "thr_val > 2^32"),
    (dict(thr_train=2**32 + 1, thr_val=2**32 + 2), "2^32"),
])
def test_split_arguments_are_validated(kw, what):
    assert _split(_args(**kw)) == -1, _err()
    assert _err().startswith("bbgr_split_edges:") and what in _err(), _err()
    # refused in a size query too: every check runs first
    n = ctypes.c_size_t(0)
    assert _lib.lib().bbgr_split_edges(ctypes.byref(_args(**kw)), None, ctypes.byref(n), None) == -1


def test_split_null_args_and_null_workspace_bytes():
    L = _lib.lib()
    n = ctypes.c_size_t(1 << 20)
    assert L.bbgr_split_edges(None, FAKE, ctypes.byref(n), None) == -1 and "null args" in _err()
    assert L.bbgr_split_edges(ctypes.byref(_args()), FAKE, None, None) == -1
    assert "workspace_bytes" in _err()


def test_a_positive_mask_stands_in_for_the_rating():
    n = ctypes.c_size_t(0)
    a = _args(rating=None, positive=FAKE)
    assert _lib.lib().bbgr_split_edges(ctypes.byref(a), None, ctypes.byref(n), None) == 0, _err()


def test_the_widest_thresholds_are_taken():
    n = ctypes.c_size_t(0)
    for thr in ((0, 0), (0, 2**32), (2**32, 2**32)):
        a = _args(thr_train=thr[0], thr_val=thr[1])
        assert _lib.lib().bbgr_split_edges(ctypes.byref(a), None, ctypes.byref(n), None) == 0


def test_workspace_query_and_small_workspace():
    n = ctypes.c_size_t(0)
    a = _args(n=1_000_000, ld_edges=1_000_000)
    assert _lib.lib().bbgr_split_edges(ctypes.byref(a), None, ctypes.byref(n), None) == 0, _err()
    # one byte per record and five int32 counts per tile of 2048 records
    tiles = -(-1_000_000 // 2048)
    assert 1_000_000 + 20 * tiles <= n.value <= 1_000_000 + 20 * tiles + (1 << 12)
    assert _split(a, FAKE, n.value - 1) == -4 and "workspace" in _err()
    assert _err().startswith("bbgr_split_edges:")


def test_split_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: n = 0 returns before any launch."""
    a = _args(n=0, n_users=0, n_items=0, user=None, item=None, rating=None, hash32=None,
              user_map=None, item_map=None, user_src=None, item_src=None, edges=None,
              counts=None, ld_edges=0)
    assert _split(a) == 0, _err()
