"""CPU: the bf16 additions to the C ABI (bbgr_to_bf16, bbgr_spmm_bf16): layout,
argument validation through ctypes (host code only: every refusal comes before
any launch), and the round-to-nearest-even rule the device kernels restate,
checked against torch's CPU conversion."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from bbgr import _lib

FAKE = 4096   # a non-null, 16-byte aligned address that is never dereferenced
INVALID, UNSUPPORTED = -1, -2


def _c_sizeof(struct_name: str, out_dir) -> int:
    src = f'#include "bbgr.h"\n#include <stdio.h>\nint main(){{printf("%zu", sizeof({struct_name}));}}'
    exe = str(out_dir / ("bbgr_sizeof_" + struct_name))   # the test's own directory
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    return int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)


def test_abi_version_is_still_12():
    assert _lib.lib().bbgr_abi_version() == 12


def test_io_struct_layout_matches_header(tmp_path):
    assert _c_sizeof("bbgr_spmm_bf16_io", tmp_path) == ctypes.sizeof(_lib.SpmmBf16Io) == 32


def test_spmm_args_layout_unchanged(tmp_path):
    # 480 bytes: the size of ABI 12's bbgr_spmm_args before the bf16 entries
    assert _c_sizeof("bbgr_spmm_args", tmp_path) == ctypes.sizeof(_lib.SpmmArgs) == 480


def _csr():
    c = _lib.CsrStruct()
    c.n_rows, c.n_cols, c.nnz = 100, 80, 1000
    c.indptr = c.indices = FAKE
    return c


def _args(**kw):
    a = _lib.SpmmArgs()
    a.d = 64
    a.y_scale_s = a.acc_scale_s = a.gamma = 1.0
    a.acc_out, a.ldacc_out = FAKE, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _io(**kw):
    h = _lib.SpmmBf16Io(FAKE, 64, FAKE, 64)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _rc(a, h, csr=None):
    L = _lib.lib()
    c = _csr() if csr is None else csr
    rc = L.bbgr_spmm_bf16(ctypes.byref(c), ctypes.byref(a), ctypes.byref(h), None)
    return rc, L.bbgr_last_error().decode()


def test_null_structs_refused():
    L = _lib.lib()
    assert L.bbgr_spmm_bf16(None, None, None, None) == INVALID
    assert b"null" in L.bbgr_last_error()
    a, c = _args(), _csr()
    assert L.bbgr_spmm_bf16(ctypes.byref(c), ctypes.byref(a), None, None) == INVALID


@pytest.mark.parametrize("d", [8, 16, 32, 48])
def test_narrow_widths_unsupported(d):
    rc, msg = _rc(_args(d=d, ldacc_out=d), _io(ldx=64, ldy=64))
    assert rc == UNSUPPORTED and f"dim {d}" in msg


@pytest.mark.parametrize("io_kw,a_kw,field", [
    (dict(x=None), {}, "null x"),
    (dict(x=FAKE + 8), {}, "x must be 16-byte aligned"),
    (dict(y=FAKE + 2), {}, "y must be 16-byte aligned"),
    (dict(ldx=68), {}, "ldx"),
    (dict(ldx=56), {}, "ldx"),
    (dict(ldy=68), {}, "ldy"),
    ({}, dict(x=FAKE, ldx=64), "args x / y must be NULL"),
    ({}, dict(y=FAKE, ldy=64), "args x / y must be NULL"),
    ({}, dict(acc_out=FAKE + 4), "acc tables"),
    ({}, dict(acc_in=FAKE, ldacc_in=66), "acc tables"),
    ({}, dict(weight_mode=1), "edge_val"),
    ({}, dict(weight_mode=3), "weight_mode"),
    ({}, dict(row_count=FAKE), "row_count needs row_list"),
])
def test_invalid_tables_refused(io_kw, a_kw, field):
    rc, msg = _rc(_args(**a_kw), _io(**io_kw))
    assert rc == INVALID and field in msg, (rc, msg)


@pytest.mark.parametrize("kw,field", [
    (dict(weight_mode=2, col_scale=FAKE), "weight_mode 2"),
    (dict(add=FAKE, ldadd=64), "add"),
    (dict(adam_param=FAKE), "adam_param"),
    (dict(adam_grad=FAKE), "adam_grad"),
    (dict(adam_mirror=FAKE), "adam_mirror"),
    (dict(src_mask=FAKE), "src_mask"),
    (dict(src_mask_bits=FAKE), "src_mask_bits"),
    (dict(src_bits=FAKE), "src_bits"),
    (dict(src_tagged=FAKE), "src_tagged"),
    (dict(tag_out=FAKE, tag_mask=FAKE), "tag_out"),
    (dict(y_map=FAKE), "y_map"),
    (dict(acc_map=FAKE), "acc_map"),
    (dict(add_map=FAKE), "add_map"),
    (dict(acc_in_map=FAKE), "acc_in_map"),
    (dict(use_range=1), "use_range"),
])
def test_unsupported_fields_refused(kw, field):
    rc, msg = _rc(_args(**kw), _io())
    assert rc == UNSUPPORTED and field in msg and "unsupported" in msg, (rc, msg)


def test_plan_without_workspace_refused():
    c = _csr()
    c.long_threshold, c.chunk_edges, c.n_chunks, c.n_split = 8, 32, 4, 1
    c.chunks = c.split = FAKE
    rc, msg = _rc(_args(), _io(), c)
    assert rc == INVALID and "partial" in msg
    rc, msg = _rc(_args(row_list=FAKE, n_row_list=4, partial=FAKE), _io(), c)
    assert rc == INVALID and "row_list needs row_mask" in msg


def test_empty_product_is_ok_without_a_launch():
    c = _csr()
    c.n_rows = c.nnz = 0
    rc, msg = _rc(_args(), _io(x=None), c)
    assert rc == 0, msg


@pytest.mark.parametrize("args,field", [
    ((-1, 64, FAKE, 64, FAKE, 64), "n_rows"),
    ((4, 66, FAKE, 68, FAKE, 72), "multiple of 4"),
    ((4, 64, None, 64, FAKE, 64), "null"),
    ((4, 64, FAKE, 64, None, 64), "null"),
    ((4, 64, FAKE + 4, 64, FAKE, 64), "src must be 16-byte aligned"),
    ((4, 64, FAKE, 66, FAKE, 64), "ldsrc"),
    ((4, 64, FAKE, 64, FAKE + 8, 64), "dst must be 16-byte aligned"),
    ((4, 64, FAKE, 64, FAKE, 68), "lddst"),
    ((4, 64, FAKE, 64, FAKE, 56), "lddst"),
])
def test_to_bf16_validates(args, field):
    L = _lib.lib()
    assert L.bbgr_to_bf16(*args, None) == INVALID
    assert field in L.bbgr_last_error().decode()
    assert L.bbgr_to_bf16(0, 64, None, 0, None, 0, None) == 0   # nothing to convert


def rne_values(n: int = 200_000, seed: int = 5) -> np.ndarray:
    """fp32 inputs of the rounding checks (shared with tests/test_gpu_bf16.py):
    normals plus +-0, subnormals, a value that rounds up to inf, +-inf and
    exact ties on both sides of even."""
    rng = np.random.default_rng(seed)
    edge = np.array([0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, 3.4e38, np.inf, -np.inf,
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),
                     1 + 2.0 ** -7, 2.0 ** -126, 2.0 ** -133], np.float32)
    return np.concatenate([rng.standard_normal(n).astype(np.float32), edge])


def rne_bits(x: np.ndarray) -> np.ndarray:
    """bf16 bit patterns of finite / infinite fp32 x, round to nearest even."""
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_rne_restatement_matches_torch_cpu():
    x = rne_values()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = rne_bits(x)
    assert np.array_equal(got, want)
    # the ties really are ties: 1 + 2^-8 -> 1 (even), 1 + 3*2^-8 -> 1 + 2^-6
    assert rne_bits(np.array([1 + 2.0 ** -8], np.float32))[0] == 0x3f80
    assert rne_bits(np.array([1 + 3 * 2.0 ** -8], np.float32))[0] == 0x3f82
