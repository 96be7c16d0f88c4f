"""CPU: bbgr_text_count and bbgr_text_unique through ctypes: the symbols
resolve, the struct layout agrees with the header, every argument is validated
and the workspace sized on the host (before any launch), and the ABI is still 12."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
SYMBOLS = ["bbgr_text_count", "bbgr_text_unique", "bbgr_text_unique_stages"]


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbols_resolve_and_abi_is_still_12():
    L = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGNATURES and s in _lib.header_symbols(), s
    assert L.bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    """sizeof and every field's offset (a swap of two same-sized fields keeps the size)."""
    names = [f[0] for f in _lib.TextArgs._fields_]
    assert names == ["n", "data", "offsets", "first", "last", "hash_mask", "n_tokens",
                     "n_unique_tokens", "recheck", "totals"]
    prints = "".join(f'printf(" %zu", offsetof(bbgr_text_args, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof(bbgr_text_args));{prints}}}')
    exe = str(tmp_path / "layout_text_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.TextArgs)
    assert [int(v) for v in out[1:]] == [getattr(_lib.TextArgs, f).offset for f in names]


def _args(**kw):
    a = _lib.TextArgs()
    a.n, a.first, a.last, a.hash_mask = 1000, 0, 350_000, 0
    a.data = a.offsets = a.n_tokens = a.n_unique_tokens = a.recheck = a.totals = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _count(a):
    return _lib.lib().bbgr_text_count(ctypes.byref(a), None)


def _unique(a, total=60_000, ws=FAKE, nbytes=1 << 40):
    n = ctypes.c_size_t(nbytes)
    return _lib.lib().bbgr_text_unique(ctypes.byref(a), total, ws, ctypes.byref(n), None)


BAD = [
    (dict(data=None), "null data"), (dict(offsets=None), "null offsets"),
    (dict(n_tokens=None), "null n_tokens"), (dict(n_unique_tokens=None), "null n_unique_tokens"),
    (dict(recheck=None), "null recheck"), (dict(totals=None), "null totals"),
    (dict(n=-1), "n out of range"), (dict(n=2**31 - 1), "n out of range"),
    (dict(first=-1), "first < 0"), (dict(first=350_001), "last < first"),
    (dict(last=2**31 - 1), "last - first out of range"),
    (dict(first=5, last=2**31 + 4), "last - first out of range"),
]


@pytest.mark.parametrize("kw,what", BAD)
def test_count_arguments_are_validated(kw, what):
    assert _count(_args(**kw)) == -1, _err()
    assert _err().startswith("bbgr_text_count:") and what in _err(), _err()


@pytest.mark.parametrize("kw,what", BAD)
def test_unique_arguments_are_validated(kw, what):
    assert _unique(_args(**kw)) == -1, _err()
    assert _err().startswith("bbgr_text_unique:") and what in _err(), _err()
    # refused in a size query too: every check runs first
    n = ctypes.c_size_t(0)
    L = _lib.lib()
    assert L.bbgr_text_unique(ctypes.byref(_args(**kw)), 60_000, None, ctypes.byref(n), None) == -1


@pytest.mark.parametrize("total", [-1, 175_501, 2**40])
def test_unique_total_tokens_is_validated(total):
    """A record of len bytes holds at most (len + 1) / 2 tokens, so 1,000 records
    in 350,000 bytes at most 175,500."""
    n = ctypes.c_size_t(0)
    for ws in (FAKE, None):
        assert _lib.lib().bbgr_text_unique(ctypes.byref(_args()), total, ws, ctypes.byref(n),
                                           None) == -1
        assert _err().startswith("bbgr_text_unique:") and "total_tokens" in _err(), _err()


def test_null_args_and_null_workspace_bytes():
    L = _lib.lib()
    n = ctypes.c_size_t(1 << 20)
    assert L.bbgr_text_count(None, None) == -1 and "null args" in _err()
    assert L.bbgr_text_unique(None, 0, FAKE, ctypes.byref(n), None) == -1 and "null args" in _err()
    assert L.bbgr_text_unique(ctypes.byref(_args()), 0, FAKE, None, None) == -1
    assert "workspace_bytes" in _err()


def test_the_widest_range_is_taken():
    n = ctypes.c_size_t(0)
    a = _args(n=2**31 - 2, first=7, last=2**31 + 5)
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), 2**31 - 2, None, ctypes.byref(n), None) == 0
    assert n.value > 32 * (2**31 - 2)
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), 2**31 - 1, None, ctypes.byref(n), None) == -1


def test_workspace_query_and_small_workspace():
    n = ctypes.c_size_t(0)
    a = _args(n=100_000, last=35_000_000)
    total = 6_000_000
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), total, None, ctypes.byref(n), None) == 0
    # per token: record, start, two hashes, two indices; per record an offset; the sort's own
    assert 32 * total + 4 * 100_001 <= n.value <= 48 * total
    assert _unique(a, total, FAKE, n.value - 1) == -4 and "workspace" in _err()
    assert _err().startswith("bbgr_text_unique:")
    # no tokens: the offsets and the library's scratch alone
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), 0, None, ctypes.byref(n), None) == 0
    assert 4 * 100_001 <= n.value < 4 << 20


def test_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: n = 0 returns before any launch, whatever the pointers."""
    a = _args(n=0, last=0, data=None, offsets=None, n_tokens=None, n_unique_tokens=None,
              recheck=None, totals=None)
    assert _count(a) == 0, _err()
    assert _unique(a, 0) == 0, _err()
    n = ctypes.c_size_t(123)
    assert _lib.lib().bbgr_text_unique(ctypes.byref(a), 0, None, ctypes.byref(n), None) == 0
    assert n.value < 4096


def test_unique_stages_checks_its_stages_and_then_as_unique():
    L = _lib.lib()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for bad in (0, -1, 8):
        assert L.bbgr_text_unique_stages(ctypes.byref(_args()), 60_000, bad, None, ctypes.byref(n),
                                         None) == -1
        assert _err().startswith("bbgr_text_unique_stages:") and "stages" in _err(), _err()
    assert L.bbgr_text_unique_stages(ctypes.byref(_args(data=None)), 60_000, 7, None,
                                     ctypes.byref(n), None) == -1
    assert _err().startswith("bbgr_text_unique_stages:") and "null data" in _err(), _err()
    # the same workspace whichever groups run
    assert L.bbgr_text_unique(ctypes.byref(_args()), 60_000, None, ctypes.byref(n), None) == 0
    for stages in (1, 2, 4, 7):
        assert L.bbgr_text_unique_stages(ctypes.byref(_args()), 60_000, stages, None,
                                         ctypes.byref(m), None) == 0
        assert m.value == n.value


@pytest.mark.parametrize("n,last,total", [(3, 3, 3), (100_000, 300_000, 200_000), (1000, 350_000, 175_500),
                                          (1, 7, 4)])
def test_record_edges_separate_without_a_byte(n, last, total):
    """Records "a", "b", "c" are three bytes and three tokens; 100,000 records
    "a b" are 300,000 bytes and 200,000 tokens: the most a call can hold is
    (last - first + n) / 2, and one more is refused."""
    nb = ctypes.c_size_t(0)
    L = _lib.lib()
    a = _args(n=n, last=last)
    assert L.bbgr_text_unique(ctypes.byref(a), total, None, ctypes.byref(nb), None) == 0, _err()
    assert nb.value >= 32 * total + 4 * (n + 1)
    assert L.bbgr_text_unique(ctypes.byref(a), total + 1, None, ctypes.byref(nb), None) == -1
    assert "total_tokens" in _err()
