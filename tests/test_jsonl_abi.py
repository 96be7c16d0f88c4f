"""CPU: the bbgr_jsonl_* entry points and bbgr_ids_number / bbgr_ids_table
through ctypes: the symbols resolve, the struct layout agrees with the header,
every argument is validated and the workspace sized on the host (before any
launch), and the ABI is still 12."""
import ctypes
import subprocess

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
SYMBOLS = ["bbgr_jsonl_count", "bbgr_jsonl_lines", "bbgr_jsonl_scan", "bbgr_jsonl_offsets",
           "bbgr_jsonl_write", "bbgr_ids_number", "bbgr_ids_table"]
POINTERS = ["data", "line_end", "item_key", "status", "rating", "helpful_vote", "verified",
            "timestamp", "ts_valid", "sizes", "spos", "totals", "offs", "side", "out_rating",
            "out_helpful", "out_verified", "out_timestamp", "out_ts_valid", "user_data", "user_off",
            "item_data", "item_off", "text_data", "text_off"]


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_symbols_resolve_and_abi_is_still_12():
    L = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGNATURES and s in _lib.header_symbols(), s
    assert L.bbgr_abi_version() == 12


def test_struct_layout_matches_header(tmp_path):
    """sizeof and every field's offset (a swap of two same-sized fields keeps the size)."""
    names = [f[0] for f in _lib.JsonlArgs._fields_]
    assert set(POINTERS) < set(names) and len(names) == 33
    prints = "".join(f'printf(" %zu", offsetof(bbgr_jsonl_args, {f}));' for f in names)
    src = (f'#include "bbgr.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           f'int main(){{printf("%zu", sizeof(bbgr_jsonl_args));{prints}}}')
    exe = str(tmp_path / "layout_jsonl_args")
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.JsonlArgs)
    assert [int(v) for v in out[1:]] == [getattr(_lib.JsonlArgs, f).offset for f in names]


def _args(**kw):
    a = _lib.JsonlArgs()
    a.n_bytes, a.n_lines, a.item_key_len = 1_000_000, 2_000, 11
    a.n_records, a.user_bytes, a.item_bytes, a.text_bytes, a.side_bytes = 1_500, 40_000, 15_000, 600_000, 64
    for p in POINTERS:
        setattr(a, p, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(fn, a, ws=FAKE, nbytes=1 << 40):
    L = _lib.lib()
    if fn in ("bbgr_jsonl_lines", "bbgr_jsonl_offsets"):
        return getattr(L, fn)(ctypes.byref(a), ws, ctypes.byref(ctypes.c_size_t(nbytes)), None)
    return getattr(L, fn)(ctypes.byref(a), None)


COMMON = [(dict(n_bytes=-1), "n_bytes out of range"), (dict(n_bytes=2**31 - 1), "n_bytes out of range"),
          (dict(data=None), "null data"), (dict(totals=None), "null totals")]
LINES = COMMON + [(dict(n_lines=-1), "n_lines out of range"),
                  (dict(n_lines=1_000_001), "n_lines out of range"),
                  (dict(line_end=None), "null line_end")]
SCAN = LINES + [(dict(**{p: None}), "null " + p) for p in
                ("status", "rating", "helpful_vote", "verified", "timestamp", "ts_valid", "sizes",
                 "spos")]
BAD = {
    "bbgr_jsonl_count": COMMON,
    "bbgr_jsonl_lines": LINES,
    "bbgr_jsonl_scan": SCAN + [(dict(item_key_len=0), "item_key_len"),
                               (dict(item_key_len=256), "item_key_len"),
                               (dict(item_key=None), "null item_key")],
    "bbgr_jsonl_offsets": SCAN + [(dict(offs=None), "null offs")],
    "bbgr_jsonl_write": SCAN + [
        (dict(offs=None), "null offs"), (dict(n_records=-1), "n_records out of range"),
        (dict(n_records=2_001), "n_records out of range"),
        (dict(user_bytes=-1), "user_bytes"), (dict(item_bytes=2**31 - 1), "item_bytes"),
        (dict(text_bytes=-1), "text_bytes"), (dict(side_bytes=-1), "side_bytes"),
        (dict(side=None), "null side"), (dict(out_helpful=None), "null output column"),
        (dict(text_off=None), "null output offsets"), (dict(item_data=None), "null output bytes")],
}


@pytest.mark.parametrize("fn,kw,what", [(fn, kw, what) for fn, bad in BAD.items() for kw, what in bad])
def test_arguments_are_validated(fn, kw, what):
    assert _call(fn, _args(**kw)) == -1, _err()
    assert _err().startswith(fn + ":") and what in _err(), _err()
    if fn in ("bbgr_jsonl_lines", "bbgr_jsonl_offsets"):     # refused in a size query too
        assert _call(fn, _args(**kw), ws=None) == -1


def test_null_args_and_null_workspace_bytes():
    L = _lib.lib()
    n = ctypes.c_size_t(1 << 20)
    for fn in SYMBOLS[:5]:
        rc = (getattr(L, fn)(None, FAKE, ctypes.byref(n), None) if fn in
              ("bbgr_jsonl_lines", "bbgr_jsonl_offsets") else getattr(L, fn)(None, None))
        assert rc == -1 and "null args" in _err() and _err().startswith(fn + ":"), fn
    for fn in ("bbgr_jsonl_lines", "bbgr_jsonl_offsets"):
        assert getattr(L, fn)(ctypes.byref(_args()), FAKE, None, None) == -1
        assert "workspace_bytes" in _err()


def test_workspace_queries_and_small_workspaces():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    a = _args(n_bytes=2**31 - 2, n_lines=50_000_000)
    assert L.bbgr_jsonl_lines(ctypes.byref(a), None, ctypes.byref(n), None) == 0, _err()
    tiles = (2**31 - 2 + 4095) // 4096
    assert 8 * tiles <= n.value < 8 * tiles + (4 << 20)      # two ints per tile, the scan's own
    assert _call("bbgr_jsonl_lines", a, FAKE, n.value - 1) == -4 and "workspace" in _err()
    assert _err().startswith("bbgr_jsonl_lines:")
    assert L.bbgr_jsonl_offsets(ctypes.byref(a), None, ctypes.byref(n), None) == 0, _err()
    assert n.value < 64 << 20          # the scans' own storage only (0 where no device answers)
    if n.value:
        assert _call("bbgr_jsonl_offsets", a, FAKE, n.value - 1) == -4 and "workspace" in _err()


def test_nothing_to_do_is_ok_without_a_launch():
    """No GPU here: an empty chunk, a chunk without lines and one without
    records return before any launch, whatever the pointers."""
    none = {p: None for p in POINTERS}
    empty = _args(n_bytes=0, n_lines=0, n_records=0, side_bytes=0, **none)
    for fn in ("bbgr_jsonl_count", "bbgr_jsonl_lines", "bbgr_jsonl_scan", "bbgr_jsonl_write"):
        assert _call(fn, empty) == 0, (fn, _err())
    no_lines = _args(n_lines=0, n_records=0, side_bytes=0, **{**none, "data": FAKE, "totals": FAKE})
    for fn in ("bbgr_jsonl_lines", "bbgr_jsonl_scan", "bbgr_jsonl_write"):
        assert _call(fn, no_lines) == 0, (fn, _err())
    assert _call("bbgr_jsonl_write", _args(n_records=0)) == 0, _err()


def _number(n=1000, data=FAKE, offsets=FAKE, data_bytes=30_000, ids=FAKE, first_rec=FAKE,
            totals=FAKE, ws=FAKE, nbytes=1 << 40):
    nb = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_ids_number(n, data, offsets, data_bytes, 0, ids, first_rec, totals, ws,
                                    ctypes.byref(nb), None)
    return rc, nb.value


@pytest.mark.parametrize("kw,what", [
    (dict(n=-1), "n out of range"), (dict(n=2**31 - 1), "n out of range"),
    (dict(data_bytes=-1), "data_bytes"), (dict(data=None), "null data"),
    (dict(offsets=None), "null offsets"), (dict(ids=None), "null ids"),
    (dict(first_rec=None), "null first_rec"), (dict(totals=None), "null totals")])
def test_ids_number_arguments_are_validated(kw, what):
    for ws in (FAKE, None):
        assert _number(ws=ws, **kw)[0] == -1
        assert _err().startswith("bbgr_ids_number:") and what in _err(), _err()


def test_ids_number_workspace():
    rc, need = _number(n=1_000_000, ws=None)
    assert rc == 0 and 44 * 1_000_000 <= need <= 64 * 1_000_000   # 44 bytes a record, the sort's own
    assert _number(n=1_000_000, nbytes=need - 1)[0] == -4 and "workspace" in _err()
    assert _number(n=2**31 - 2, ws=None)[0] == 0
    rc, need = _number(n=0, data=None, offsets=None, ids=None, first_rec=None, totals=None)
    assert rc == 0                                            # nothing to do: no launch
    L = _lib.lib()
    assert L.bbgr_ids_number(5, FAKE, FAKE, 9, 0, FAKE, FAKE, FAKE, FAKE, None, None) == -1
    assert "workspace_bytes" in _err()


def _table(n_ids=100, first_rec=FAKE, n=1000, data=FAKE, offsets=FAKE, data_bytes=30_000,
           tab_offsets=FAKE, tab_data=FAKE, tab_bytes=3_000, ws=FAKE, nbytes=1 << 40):
    nb = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_ids_table(n_ids, first_rec, n, data, offsets, data_bytes, tab_offsets,
                                   tab_data, tab_bytes, ws, ctypes.byref(nb), None)
    return rc, nb.value


@pytest.mark.parametrize("kw,what", [
    (dict(n=-1), "n out of range"), (dict(n=2**31 - 1), "n out of range"),
    (dict(n_ids=-1), "n_ids out of range"), (dict(n_ids=1001), "n_ids out of range"),
    (dict(data_bytes=-1), "data_bytes"), (dict(tab_bytes=-1), "tab_bytes"),
    (dict(tab_bytes=30_001), "tab_bytes"), (dict(tab_offsets=None), "null tab_offsets"),
    (dict(first_rec=None), "null first_rec"), (dict(data=None), "null data"),
    (dict(offsets=None), "null offsets")])
def test_ids_table_arguments_are_validated(kw, what):
    for ws in (FAKE, None):
        assert _table(ws=ws, **kw)[0] == -1
        assert _err().startswith("bbgr_ids_table:") and what in _err(), _err()


def test_ids_table_workspace_and_nothing_to_do():
    rc, need = _table(ws=None)
    assert rc == 0 and need < 4 << 20  # the scan's own storage only (0 where no device answers)
    if need:
        assert _table(nbytes=need - 1)[0] == -4 and "workspace" in _err()
    assert _table(n_ids=0, first_rec=None, data=None, offsets=None, tab_bytes=0)[0] == 0, _err()
    assert _table(tab_bytes=0)[0] == 0, _err()               # an empty table: no launch
