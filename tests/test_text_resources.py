"""CPU: the text kernels of the built gfx950 code object use no scratch (the
metadata read by tools/kernel_resources.py): the per-token kernels walk bytes
in loops whose state must stay in registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources as KR  # noqa: E402

KERNELS = ["text_walk_kernelILb0E", "text_walk_kernelILb1E", "text_hash_kernel",
           "text_verify_kernel", "text_recheck_total_kernel"]


def test_text_kernels_use_no_scratch():
    objs = [o for o in KR.product_objects() if os.path.basename(o) == "text.o"]
    if not objs and not os.path.exists(os.path.join(KR.PKG, "lib", "libbbgr.so")):
        pytest.skip("build() has not run (no lib/libbbgr.so)")
    assert objs, "libbbgr.so was built without csrc/text.hip (no lib/obj/text.o)"
    ours = {k: v for k, v in KR.kernels(objs[0]).items() if k.startswith("_ZN4bbgr")}
    for want in KERNELS:
        assert any(want in k for k in ours), (want, sorted(ours))
    assert len(ours) == len(KERNELS), sorted(ours)
    for name, r in ours.items():
        assert r["scratch"] == 0, (name, r)
