"""The workspace protocol of include/bbgr.h, the same for every entry point that
takes (void *workspace, size_t *workspace_bytes): a null workspace_bytes is
refused by name, a null workspace asks for the size, and a workspace one byte
short is refused with the one text "<entry>: workspace <have> < <need> bytes",
<entry> being the exported name the caller used. The entry list and the
arguments are those of tools/workspace_sizes.py (fake non-null pointers:
nothing is read or launched).

hipcub's own sizing of some primitives asks the runtime for a device, so the
size query of the entries in DEVICE_QUERIES answers BBGR_ERR_HIP (or, where
hipcub's size is all there is, 0 bytes) on a host without one: those run
where a GPU is present, still without a launch."""
import ctypes
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
WS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(WS)

from bbgr import _lib  # noqa: E402

INVALID, WORKSPACE = -1, -4
DEVICE_QUERIES = WS.DEVICE_QUERIES
HOST_QUERIES = sorted(set(WS.CASES) - set(DEVICE_QUERIES))


def _err():
    return _lib.lib().bbgr_last_error().decode()


def _protocol(entry):
    _, before = WS.CASES[entry][0]   # the tiny shape
    assert WS.run(entry, before, WS.FAKE, None) == INVALID, _err()
    assert "workspace_bytes" in _err() and _err().startswith(entry + ":"), _err()
    need = ctypes.c_size_t(0)
    assert WS.run(entry, before, None, need) == 0, _err()
    assert need.value > 0
    have = ctypes.c_size_t(need.value - 1)
    assert WS.run(entry, before, WS.FAKE, have) == WORKSPACE, _err()
    assert _err() == f"{entry}: workspace {need.value - 1} < {need.value} bytes"
    assert have.value == need.value - 1   # a refusal leaves the caller's size alone


def test_every_workspace_entry_is_listed():
    """The table covers each entry point whose signature has a size_t pointer."""
    takes_ws = {name for name, (argtypes, _) in _lib._SIGNATURES.items()
                if ctypes.POINTER(ctypes.c_size_t) in argtypes}
    assert takes_ws == set(WS.CASES)
    assert all(len(cases) == 2 for cases in WS.CASES.values())


@pytest.mark.parametrize("entry", HOST_QUERIES)
def test_protocol(entry):
    _protocol(entry)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", DEVICE_QUERIES)
def test_protocol_of_queries_that_need_a_device(entry):
    _protocol(entry)
