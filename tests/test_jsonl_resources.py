"""CPU: the review-dump kernels of the built gfx950 code object use no scratch
(the metadata read by tools/kernel_resources.py): the scan and the string
walk keep their state, the eight value positions included, in registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources as KR  # noqa: E402

KERNELS = ["jsonl_tile_kernelILb0E", "jsonl_tile_kernelILb1E", "jsonl_scan_kernel",
           "jsonl_write_kernel", "ids_hash_kernel", "ids_verify_kernel", "ids_heads_kernel",
           "ids_assign_kernel", "ids_table_kernel"]


def test_jsonl_kernels_use_no_scratch():
    objs = [o for o in KR.product_objects() if os.path.basename(o) == "jsonl.o"]
    if not objs and not os.path.exists(os.path.join(KR.PKG, "lib", "libbbgr.so")):
        pytest.skip("build() has not run (no lib/libbbgr.so)")
    assert objs, "libbbgr.so was built without csrc/jsonl.hip (no lib/obj/jsonl.o)"
    ours = {k: v for k, v in KR.kernels(objs[0]).items() if k.startswith("_ZN4bbgr")}
    for want in KERNELS:
        assert any(want in k for k in ours), (want, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, r in ours.items():
        assert r["scratch"] == 0, (name, r)
