"""CPU: the error bound behind recommend(precision="bf16_exact").

|s^ - s| <= eps(d) ||u|| ||i||, eps(d) = 1.02 * 2^-7 + d * 2^-21, where s^ is the
fp32-accumulated score of the bf16-rounded rows and s the fp32 fma chain of
bbgr_recommend (oracle_score_chain's order: components 0, d/2, 1, d/2+1, ...).

The operand term is 2^-7, not the 2^-8 first proposed for it: bf16 keeps 8
significant bits, so one rounding errs by up to 2^-8 (1 + 2^-8 is a midpoint),
two operands by 2 * 2^-8 + 2^-16. The midpoint tables below reach 0.0078 =
2^-7 of ||u|| ||i|| on rows of one sign, twice what 1.02 * 2^-8 + d * 2^-21 =
0.0040 would allow (test_bound_on_rounding_midpoints asserts both).

s is computed here by a vectorised float32 chain whose every fma is exact
products and sums in float64 rounded once to float32 (a product of two fp32 has
48 bits; the sum with an fp32 accumulator is rounded by float64 first, a double
rounding that can differ from fmaf in the last bit: one fp32 ulp of a partial
sum, which the test adds to what it allows, d * 2^-24 of sum |u_c||i_c| at
most); a sample of pairs is checked against oracle_score_chain itself. s^ is
taken in two accumulation orders (ascending components, and 16-component blocks
as the bf16 MFMA consumes them), each fp32-rounded per addition; the norms are
float64.
"""
import numpy as np
import pytest
import torch

from bbgr import recommend as RC

WIDTHS = (64, 128, 256)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def _chain32(u, it):
    """[nu, ni] float32: the fp32 chain per pair, components 0, d/2, 1, ..."""
    h = u.shape[1] // 2
    acc = np.zeros((u.shape[0], it.shape[0]), np.float32)
    u64, i64 = u.astype(np.float64), it.astype(np.float64)
    for s in range(h):
        for c in (s, h + s):
            acc = (acc.astype(np.float64) + np.outer(u64[:, c], i64[:, c])).astype(np.float32)
    return acc


def _bf16_scores(uh, ih, block):
    """fp32-accumulated scores of bf16-valued rows: exact products, exact sums
    inside a block of `block` components, one fp32 rounding per block."""
    d = uh.shape[1]
    acc = np.zeros((uh.shape[0], ih.shape[0]), np.float32)
    u64, i64 = uh.astype(np.float64), ih.astype(np.float64)
    for c0 in range(0, d, block):
        acc = (acc.astype(np.float64) + u64[:, c0:c0 + block] @ i64[:, c0:c0 + block].T
               ).astype(np.float32)
    return acc


def _check(u, it, d):
    eps = RC.bf16_error_bound(d)
    s = _chain32(u, it).astype(np.float64)
    uh, ih = _bf16(u), _bf16(it)
    nn = np.outer(np.linalg.norm(u.astype(np.float64), axis=1),
                  np.linalg.norm(it.astype(np.float64), axis=1))
    absdot = np.abs(u.astype(np.float64)) @ np.abs(it.astype(np.float64)).T
    slack = d * 2.0 ** -24 * absdot       # the float64 stand-in for fmaf (docstring)
    worst = 0.0
    for block in (1, 16):
        sh = _bf16_scores(uh, ih, block).astype(np.float64)
        err = np.abs(sh - s)
        assert (err <= eps * nn + slack).all(), (d, block, (err / nn).max())
        worst = max(worst, float((err / np.maximum(nn, 1e-300)).max()))
    return worst


def test_error_bound_formula():
    for d in (8, 64, 128, 256):
        assert RC.bf16_error_bound(d) == 1.02 * 2.0 ** -7 + d * 2.0 ** -21
    assert 0.0079 < RC.bf16_error_bound(64) < RC.bf16_error_bound(256) < 0.0082


@pytest.mark.parametrize("d", WIDTHS)
def test_chain_stand_in_matches_the_oracle_chain(d):
    """The vectorised chain is oracle_score_chain to within the double-rounding
    slack the bound tests allow (equal bits on all but a few pairs)."""
    from oracle import native as N
    rng = np.random.default_rng(1000 + d)
    u = rng.uniform(-0.3, 0.3, (8, d)).astype(np.float32)
    it = rng.uniform(-0.3, 0.3, (40, d)).astype(np.float32)
    got = _chain32(u, it)
    want = np.array([[N.score_chain(a, b) for b in it] for a in u], np.float32)
    absdot = np.abs(u.astype(np.float64)) @ np.abs(it.astype(np.float64)).T
    assert (np.abs(got.astype(np.float64) - want) <= d * 2.0 ** -24 * absdot).all()
    assert (got == want).mean() > 0.9


@pytest.mark.parametrize("d", WIDTHS)
def test_bound_on_the_uniform_tables(d):
    """The tables of tests/test_gpu_recommend.py (same generator and seed)."""
    rng = np.random.default_rng(1000 + d)
    u = rng.uniform(-0.3, 0.3, (300, d)).astype(np.float32)
    it = rng.uniform(-0.3, 0.3, (1500, d)).astype(np.float32)
    worst = _check(u, it, d)
    print(f"d={d}: max |s^-s| / (|u||i|) = {worst:.5f}, eps = {RC.bf16_error_bound(d):.5f}")
    assert worst < 0.002    # well inside: random signs cancel (0.0015 / 0.0011 / 0.0008)


@pytest.mark.parametrize("d", WIDTHS)
def test_bound_on_spread_magnitudes(d):
    """Row and component magnitudes spread over 2^-20 ... 2^20: the bound is
    relative to the norms, so a few large components dominate both sides."""
    rng = np.random.default_rng(7 + d)
    def table(n):
        mant = rng.uniform(1.0, 2.0, (n, d)) * rng.choice([-1.0, 1.0], (n, d))
        comp = rng.integers(-20, 21, (n, d))
        comp[::2] = rng.integers(-20, 21, (n + 1) // 2)[:, None]   # every other row: one scale
        return (mant * 2.0 ** comp).astype(np.float32)
    _check(table(120), table(400), d)


@pytest.mark.parametrize("d", WIDTHS)
def test_bound_on_rounding_midpoints(d):
    """Every component sits on a bf16 rounding midpoint, (1 + (2 m + 1) 2^-8)
    2^e with both signs: each operand carries the largest rounding error there
    is, and ties-to-even sends neighbours opposite ways."""
    rng = np.random.default_rng(11 + d)
    def table(n):
        m = rng.integers(0, 64, (n, d))
        e = rng.integers(-3, 4, (n, d))
        sign = rng.choice([-1.0, 1.0], (n, d))
        v = (sign * (1.0 + (2 * m + 1) * 2.0 ** -8) * 2.0 ** e).astype(np.float32)
        v[0] = 1.0 + 2.0 ** -8          # the plain 1 + 2^-8 pattern, all one sign
        v[1] = -(1.0 + 2.0 ** -8)
        v[2] = (1.0 + 3 * 2.0 ** -8)    # rounds up (to even), where 1 + 2^-8 rounds down
        return v
    u, it = table(100), table(300)
    # they are midpoints: the bf16 value differs by exactly half a bf16 ulp
    rel = np.abs(_bf16(u).astype(np.float64) - u) / np.abs(u)
    assert rel.min() > 2.0 ** -9 and rel.max() <= 2.0 ** -8
    worst = _check(u, it, d)
    print(f"d={d}: max |s^-s| / (|u||i|) = {worst:.5f}")
    # the operand term is reached: rows 0 / 1 round every component the same way
    assert worst > 0.99 * 2.0 ** -7 > 1.02 * 2.0 ** -8 + d * 2.0 ** -21


def test_default_prefilter_rule():
    want = {1: 32, 16: 32, 17: 34, 64: 128, 65: 128, 128: 128}
    for k, kp in want.items():
        assert RC.default_prefilter_k(k) == kp == min(128, max(32, 2 * k))
        assert k <= kp <= 128
