"""CPU: bbgr_text_gather through ctypes: the symbol resolves, the struct layout
agrees with the header, every argument is validated and the workspace sized
on the host (before any launch), and the ABI is still 12."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
FN = "bbgr_text_gather"


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbol_resolves_and_abi_is_still_12():
    L = _lib.lib()
    assert hasattr(L, FN) and FN in _lib._SIGNATURES and FN in _lib.header_symbols()
    assert L.bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    """sizeof and every field's offset (a swap of two same-sized fields keeps the size)."""
    names = [f[0] for f in _lib.TextGatherArgs._fields_]
    assert names == ["n_list", "records", "n", "data", "offsets", "first", "last", "out_offsets",
                     "out_data", "capacity", "total"]
    prints = "".join(f'printf(" %zu", offsetof(bbgr_text_gather_args, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof(bbgr_text_gather_args));{prints}}}')
    exe = str(tmp_path / "layout_text_gather_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.TextGatherArgs)
    assert [int(v) for v in out[1:]] == [getattr(_lib.TextGatherArgs, f).offset for f in names]


def _args(**kw):
    a = _lib.TextGatherArgs()
    a.n_list, a.n, a.first, a.last, a.capacity = 1000, 5000, 0, 350_000, 1 << 20
    a.records = a.data = a.offsets = a.out_offsets = a.out_data = a.total = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _gather(a, ws=FAKE, nbytes=1 << 40):
    n = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_text_gather(None if a is None else ctypes.byref(a), ws, ctypes.byref(n),
                                     None)
    return rc, n.value


BAD = [
    (dict(records=None), "null records"), (dict(data=None), "null data"),
    (dict(offsets=None), "null offsets"), (dict(out_offsets=None), "null out_offsets"),
    (dict(total=None), "null total"),
    (dict(n_list=-1), "n_list out of range"), (dict(n_list=2**31 - 1), "n_list out of range"),
    (dict(n=-1), "n < 0"), (dict(first=-1), "first < 0"), (dict(first=350_001), "last < first"),
    (dict(capacity=-1), "capacity < 0"),
    (dict(out_data=FAKE + 8), "out_data must be 16-byte aligned"),
    (dict(out_data=FAKE + 1), "out_data must be 16-byte aligned"),
]


@pytest.mark.parametrize("kw,what", BAD)
def test_arguments_are_validated(kw, what):
    for ws in (FAKE, None):                   # refused in a size query too: every check runs first
        rc, _ = _gather(_args(**kw), ws=ws)
        assert rc == -1, _err()
        assert _err().startswith(FN + ":") and what in _err(), _err()


def test_null_args_and_null_workspace_bytes():
    rc, _ = _gather(None)
    assert rc == -1 and _err().startswith(FN + ":") and "null args" in _err()
    assert _lib.lib().bbgr_text_gather(ctypes.byref(_args()), FAKE, None, None) == -1
    assert _err().startswith(FN + ":") and "workspace_bytes" in _err()


def test_what_is_not_limited():
    """The source text and the capacity may pass 2^31 - 1 bytes, out_data may
    be null (offsets and total only), and a text without a record needs no
    bytes."""
    for kw in (dict(first=7, last=2**40), dict(capacity=2**40), dict(out_data=None),
               dict(out_data=None, capacity=0), dict(n=0, data=None, offsets=None),
               dict(n_list=2**31 - 2)):
        rc, nb = _gather(_args(**kw), ws=None, nbytes=0)
        assert rc == 0 and nb > 0, _err()


def test_workspace_query_and_small_workspace():
    rc, nb = _gather(_args(n_list=100_000), ws=None, nbytes=0)
    assert rc == 0, _err()
    assert 8 * 100_000 <= nb < 8 * 100_000 + (4 << 20)     # a length per listed record, the scan's own
    rc, _ = _gather(_args(n_list=100_000), nbytes=nb - 1)
    assert rc == -4 and _err() == f"{FN}: workspace {nb - 1} < {nb} bytes"
    rc, nb1 = _gather(_args(n_list=1), ws=None, nbytes=0)
    assert rc == 0 and 8 <= nb1 < 4 << 20


def test_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: n_list = 0 returns before any launch, whatever the pointers."""
    a = _args(n_list=0, n=0, last=0, capacity=0, records=None, data=None, offsets=None,
              out_offsets=None, out_data=None, total=None)
    rc, _ = _gather(a)
    assert rc == 0, _err()
    rc, nb = _gather(a, ws=None, nbytes=123)
    assert rc == 0 and nb < 4096


def test_the_measurement_entry_checks_its_fetch_and_then_as_gather():
    """bbgr_text_gather_fetch: the symbol, the fetch forms 0 and 1, the same
    checks under its own name and the same workspace."""
    L = _lib.lib()
    name = "bbgr_text_gather_fetch"
    assert hasattr(L, name) and name in _lib._SIGNATURES and name in _lib.header_symbols()
    assert _lib.TEXT_FETCH == {"unaligned": 0, "aligned_pair": 1}
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for bad in (-1, 2, 7):
        assert L.bbgr_text_gather_fetch(ctypes.byref(_args()), bad, None, ctypes.byref(n), None) == -1
        assert _err().startswith(name + ":") and "fetch out of range" in _err(), _err()
    assert L.bbgr_text_gather_fetch(ctypes.byref(_args(records=None)), 1, None, ctypes.byref(n),
                                    None) == -1
    assert _err().startswith(name + ":") and "null records" in _err(), _err()
    assert L.bbgr_text_gather(ctypes.byref(_args()), None, ctypes.byref(n), None) == 0
    for fetch in (0, 1):
        assert L.bbgr_text_gather_fetch(ctypes.byref(_args()), fetch, None, ctypes.byref(m), None) == 0
        assert m.value == n.value
