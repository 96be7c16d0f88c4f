"""GPU: bbgr_text_gather (csrc/text_gather.hip) against numpy concatenation,
byte for byte: record lengths around the 16-byte word, the 64-byte line, the
1 KiB tile of a wave and one of 1 MiB, every alignment of source and
destination, lists in any order with repeats and ids outside the text,
``first`` / ``last`` cutting into the first and last record, a capacity short
of the total, a null output, and source addresses beyond 2^31 and 2^32; the
same through bbgr_text_gather_fetch with either source fetch."""
import ctypes

import numpy as np
import pytest
import torch

from bbgr import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0xA5
LENGTHS = [257, 0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 1023, 1024, 1025, 4095, 4096, 4097]
BIG = 1 << 20


FETCHES = [None, "unaligned", "aligned_pair"]   # bbgr_text_gather; bbgr_text_gather_fetch's two


def gather(records, data, offsets, first, last, capacity, out=None, null_out=False, fetch=None):
    """One call on device tensors: (out_offsets, total, out), the output
    buffer `capacity` + 64 bytes of SENTINEL unless given. `fetch`: None for
    bbgr_text_gather, else the form bbgr_text_gather_fetch is to use."""
    rec = torch.as_tensor(np.asarray(records, np.int32)).to(DEV)
    m = rec.numel()
    out_off = torch.full((m + 1,), -1, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    if out is None and not null_out:
        out = torch.full((capacity + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    a = _lib.TextGatherArgs()
    a.n_list, a.records, a.n = m, rec.data_ptr(), offsets.numel() - 1
    a.data, a.offsets, a.first, a.last = data.data_ptr(), offsets.data_ptr(), first, last
    a.out_offsets, a.out_data = out_off.data_ptr(), None if null_out else out.data_ptr()
    a.capacity, a.total = capacity, total.data_ptr()
    if fetch is None:
        _lib.call_with_workspace("bbgr_text_gather", ctypes.byref(a), device=DEV)
    else:
        _lib.call_with_workspace("bbgr_text_gather_fetch", ctypes.byref(a), _lib.TEXT_FETCH[fetch],
                                 device=DEV)
    return out_off.cpu().numpy(), int(total), out


@pytest.fixture(scope="module")
def source():
    """Records of LENGTHS, 64 short ones of mixed lengths that move the starts
    over every residue mod 16, and one of 1 MiB in the middle: host bytes and
    offsets, and both on the device. Record 0 and the last are long enough for
    `first` / `last` to cut into them."""
    rng = np.random.default_rng(7)
    lens = (LENGTHS + rng.integers(0, 40, 32).tolist() + [BIG]
            + rng.integers(0, 40, 32).tolist() + [65])
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    starts = off[:-1][np.asarray(lens) > 0]
    assert set((starts % 16).tolist()) == set(range(16))
    return data, off, torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)


def _expected(records, data, off, first, last):
    n = off.size - 1
    parts, lens = [], []
    for r in records:
        if 0 <= r < n:
            b, e = max(int(off[r]), first), min(int(off[r + 1]), last)
            e = max(e, b)
        else:
            b = e = 0
        parts.append(data[b:e])
        lens.append(e - b)
    want_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=want_off[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), want_off


def _lists(n, big):
    rng = np.random.default_rng(3)
    small = np.asarray([r for r in range(n) if r != big])
    order = np.arange(n)
    lists = {"in order": order, "reversed": order[::-1].copy(),
             "repeats": np.concatenate([rng.choice(small, 200), [big, 5, big], rng.choice(small, 50)]),
             "ids outside": np.concatenate([[-1], order[:40], [n, 2**31 - 5, -7], order[40:],
                                            [2**31 - 5]])}
    for m in (1, 63, 64, 65, 8193):
        lists[f"{m} ids"] = rng.choice(small, m)
    lists["1 id, the long record"] = np.asarray([big])
    return lists


@pytest.mark.parametrize("fetch", FETCHES)
def test_lists_against_concatenation(source, fetch):
    data, off, d_dev, o_dev = source
    n = off.size - 1
    big = int(np.argmax(np.diff(off)))
    first, last = int(off[0]), int(off[-1])
    for name, records in _lists(n, big).items():
        want, want_off = _expected(records.tolist(), data, off, first, last)
        total = int(want_off[-1])
        got_off, got_total, out = gather(records, d_dev, o_dev, first, last, total + 16, fetch=fetch)
        assert got_off.tolist() == want_off.tolist(), name
        assert got_total == total, name
        got = out.cpu().numpy()
        assert got[:total].tobytes() == want.tobytes(), name
        assert (got[total:] == SENTINEL).all(), name          # nothing behind total
        if name == "in order":
            dst = want_off[:-1][np.diff(want_off) > 0]
            assert set((dst % 16).tolist()) == set(range(16))
        # a second call into a fresh buffer of sentinels: the same bytes, all of them written
        _, _, again = gather(records, d_dev, o_dev, first, last, total + 16, fetch=fetch)
        assert again.data_ptr() != out.data_ptr() and torch.equal(again, out), name


@pytest.mark.parametrize("fetch", FETCHES)
@pytest.mark.parametrize("cut", [(3, 5), (200, 60), (257, 65), (1, 0), (0, 1)])
def test_first_and_last_cut_into_the_records(source, cut, fetch):
    """No byte before `first` or from `last` on is copied; a record that the
    cut leaves nothing of is empty."""
    data, off, d_dev, o_dev = source
    n = off.size - 1
    first, last = int(off[0]) + cut[0], int(off[-1]) - cut[1]
    records = np.concatenate([np.arange(n), [0, n - 1, 0]])
    want, want_off = _expected(records.tolist(), data, off, first, last)
    total = int(want_off[-1])
    got_off, got_total, out = gather(records, d_dev, o_dev, first, last, total, fetch=fetch)
    assert got_off.tolist() == want_off.tolist() and got_total == total
    got = out.cpu().numpy()
    assert got[:total].tobytes() == want.tobytes() and (got[total:] == SENTINEL).all()


@pytest.mark.parametrize("fetch", FETCHES)
def test_text_that_ends_with_the_buffer(fetch):
    """The last 16 bytes below `last` are read one by one, not with a 16-byte
    load that would pass it: records that end there at every length below 33."""
    rng = np.random.default_rng(5)
    for tail in range(1, 33):
        lens = [21, tail]
        off = np.asarray([0, 21, 21 + tail], np.int64)
        data = rng.integers(0, 256, sum(lens), dtype=np.uint8)
        d_dev, o_dev = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)
        want, want_off = _expected([1, 0, 1], data, off, 0, int(off[-1]))
        got_off, total, out = gather([1, 0, 1], d_dev, o_dev, 0, int(off[-1]), int(want_off[-1]),
                                     fetch=fetch)
        assert got_off.tolist() == want_off.tolist() and total == want_off[-1]
        assert out.cpu().numpy()[:total].tobytes() == want.tobytes(), tail


def test_a_short_capacity_and_a_null_output(source):
    data, off, d_dev, o_dev = source
    n = off.size - 1
    first, last = int(off[0]), int(off[-1])
    records = np.arange(n)[::-1].copy()
    want, want_off = _expected(records.tolist(), data, off, first, last)
    total = int(want_off[-1])
    for capacity in (total - 7, total - 16, 1000, 5, 0):
        got_off, got_total, out = gather(records, d_dev, o_dev, first, last, capacity)
        assert got_off.tolist() == want_off.tolist() and got_total == total     # in full
        got = out.cpu().numpy()
        assert got[:capacity].tobytes() == want[:capacity].tobytes(), capacity
        assert (got[capacity:] == SENTINEL).all(), capacity   # nothing at or behind capacity
    got_off, got_total, _ = gather(records, d_dev, o_dev, first, last, 0, null_out=True)
    assert got_off.tolist() == want_off.tolist() and got_total == total


def test_no_record_has_a_byte(source):
    data, off, d_dev, o_dev = source
    got_off, total, out = gather([-1, 1, 2**31 - 5, 1], d_dev, o_dev, 0, int(off[-1]), 64)
    assert got_off.tolist() == [0] * 5 and total == 0
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("fetch", FETCHES)
def test_source_addresses_beyond_32_bits(fetch):
    """A text of 2^32 + 2^20 zero bytes made on the device; forty short records
    written into it near 0, across 2^31 - 1 | 2^31, across 2^32 - 1 | 2^32 and
    up to its last byte, with the zeros between them as records of their own."""
    N = 2**32 + 2**20
    rng = np.random.default_rng(9)
    data = torch.zeros(N, dtype=torch.uint8, device=DEV)
    spans = []
    for k in range(10):
        spans.append((100 * k + k, 100 * k + k + int(rng.integers(1, 60))))            # near 0
    for edge in (2**31, 2**32):
        at = edge - 700                                        # before the edge
        for k in range(8):
            ln = int(rng.integers(17, 60))
            spans.append((at, at + ln))
            at += ln + int(rng.integers(0, 9))
        spans += [(edge - 60, edge - 30), (edge - 30, edge - 9),
                  (edge - 9, edge + 13),                       # across it
                  (edge + 13, edge + 14), (edge + 14, edge + 47)]
    for k in range(5):
        spans.append((N - 200 + 40 * k, N - 200 + 40 * k + 33))
    spans[-1] = (spans[-1][0], N)                              # ends with the tensor
    spans = sorted(set(spans))
    bounds = sorted({0, N} | {b for s in spans for b in s})
    off = np.asarray(bounds, np.int64)
    real = [int(np.searchsorted(off, a)) for a, _ in spans]   # record ids of the written spans
    assert len(real) >= 40 and all(off[r + 1] == b for r, (_, b) in zip(real, spans))
    assert any(a < 2**31 <= b - 1 for a, b in spans) and any(a < 2**32 <= b - 1 for a, b in spans)
    want = {}
    for r, (a, b) in zip(real, spans):
        want[r] = rng.integers(1, 256, b - a, dtype=np.uint8)
        data[a:b] = torch.from_numpy(want[r]).to(DEV)
    o_dev = torch.from_numpy(off).to(DEV)
    order = rng.permutation(real).tolist() + [real[0], real[-1]]
    expect = np.concatenate([want[r] for r in order])
    got_off, total, out = gather(order, data, o_dev, 0, N, expect.size, fetch=fetch)
    assert total == expect.size
    assert got_off.tolist() == np.cumsum([0] + [want[r].size for r in order]).tolist()
    assert out.cpu().numpy()[:total].tobytes() == expect.tobytes()
    assert bool((out[total:] == SENTINEL).all())
