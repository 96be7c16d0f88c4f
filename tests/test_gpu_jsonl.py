"""GPU: bbgr.jsonl.read_reviews against the host reader
(features.review_columns_from_jsonl, tokens="device"), bit for bit: every
column, the text, both id tables and the token counts, on the corpora of
tests/jsonl_ref.py and on inputs built to put every token kind across the
64-byte steps of the scan; chunking, device input, the host fallback, the
numbering fallback, and the consumers downstream."""
import numpy as np
import pytest
import torch

import jsonl_ref as R
from bbgr import jsonl
from bbgr.features import build_credibility_graph, review_columns_from_jsonl
from bbgr.split import split_interactions

pytestmark = pytest.mark.gpu

COLUMNS = ("user", "item", "rating", "helpful_vote", "verified", "timestamp", "ts_valid",
           "n_tokens", "n_unique_tokens")


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _table(d: dict):
    enc = [s.encode("utf-8", "surrogatepass") for s in d]
    return b"".join(enc), np.cumsum([0] + [len(b) for b in enc]).astype(np.int64)


def _host(tmp_path, data: bytes, name="host.jsonl", key="parent_asin"):
    p = tmp_path / name
    p.write_bytes(data)
    return review_columns_from_jsonl(str(p), key, tokens="device")


def _assert_equal(parsed, host):
    cols, user2idx, item2idx = host
    assert len(parsed.cols) == len(cols)
    for name in COLUMNS:
        got, want = _np(getattr(parsed.cols, name)), _np(getattr(cols, name))
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert got.tobytes() == want.tobytes(), name
    assert isinstance(parsed.cols.text.data, torch.Tensor) and parsed.cols.text.data.is_cuda
    assert _np(parsed.cols.text.data).tobytes() == _np(cols.text.data).tobytes()
    assert _np(parsed.cols.text.offsets).tolist() == _np(cols.text.offsets).tolist()
    for got, want in ((parsed.user_ids, user2idx), (parsed.item_ids, item2idx)):
        data, off = _table(want)
        assert _np(got.data).tobytes() == data
        assert _np(got.offsets).dtype == np.int64 and _np(got.offsets).tolist() == off.tolist()
    assert parsed.info["records"] == len(cols)


def _check(tmp_path, data: bytes, **kw):
    parsed = jsonl.read_reviews(data, **kw)
    _assert_equal(parsed, _host(tmp_path, data, key=kw.get("item_id_key", "parent_asin")))
    return parsed


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    data = R.plain_corpus()
    return data, _host(tmp_path_factory.mktemp("plain"), data)


@pytest.fixture(scope="module")
def odd(tmp_path_factory):
    data = R.odd_corpus()
    return data, _host(tmp_path_factory.mktemp("odd"), data)


def test_plain_corpus(plain, tmp_path):
    data, host = plain
    p = tmp_path / "plain.jsonl"
    p.write_bytes(data)
    parsed = jsonl.read_reviews(str(p))                      # a path: memory-mapped
    _assert_equal(parsed, host)
    ref = R.parse(data, "parent_asin", jsonl.host_record)
    assert parsed.info["flagged"] == 0 == ref["flagged"]
    for k in ("lines", "records", "blank", "skipped"):
        assert parsed.info[k] == ref[k], k
    assert parsed.info["numbering_fallback"] == 0 and parsed.info["chunks"] == 1
    assert jsonl.id_dict(parsed.user_ids) == host[1] and jsonl.id_dict(parsed.item_ids) == host[2]


def test_odd_corpus(odd):
    data, host = odd
    parsed = jsonl.read_reviews(bytearray(data))
    _assert_equal(parsed, host)
    ref = R.parse(data, "parent_asin", jsonl.host_record)
    for k in ("lines", "records", "blank", "skipped", "flagged"):
        assert parsed.info[k] == ref[k], k
    assert ref["flagged"] >= 20


def test_another_item_key(tmp_path):
    data = (b'{"user_id":"u","asin":"A","parent_asin":"P","rating":4}\n'
            b'{"user_id":"u","asin":"B","parent_asin":"P","rating":5,"user_id":"w"}\n')
    assert len(_check(tmp_path, data, item_id_key="asin").item_ids) == 2
    assert len(_check(tmp_path, data, item_id_key="user_id").item_ids) == 2
    with pytest.raises(ValueError):
        jsonl.read_reviews(data, item_id_key='a"b')


def test_a_line_at_each_of_the_64_alignments(tmp_path):
    lines, at, starts = [], 0, set()
    for k in range(130):
        line = b'{"user_id":"u%d","parent_asin":"i%d","rating":%d.5,"text":"%s"}' % (
            k % 7, k % 5, k % 5, b"w" * k)
        starts.add(at % 64)
        at += len(line) + 1
        lines.append(line)
    assert starts == set(range(64))
    _check(tmp_path, b"\n".join(lines) + b"\n")


def test_every_token_kind_across_a_step_edge_at_every_phase(tmp_path):
    """The scan steps through a line 64 bytes at a time from its first byte: a
    pad of 0 .. 139 bytes before them moves a backslash run of odd and of even
    length, a \\uXXXX escape, a surrogate pair, a key name, a number literal, a
    closing quote and the '":"' after a key over every phase of a step edge
    (the longest, the pair, has 12 bytes; the tokens lie within 200 bytes)."""
    tail = (b'"user_id":"u\\\\\\"x\\\\\\\\","verified_purchase":true,"timestamp":1588687728923,'
            b'"parent_asin":"i\\u00e9\\ud83d\\ude00","helpful_vote":12345,"rating":4.25,'
            b'"title":"t\\\\","text":"a\\"b \\u20ac \\uD83D\\uDC4D end\\\\\\\\"}')
    lines = [b'{"pad":"' + b"p" * k + b'",' + tail for k in range(140)]
    lines += [b'{"pad":"' + b"\\\\" * k + b'",' + tail for k in range(40)]
    parsed = _check(tmp_path, b"\n".join(lines))
    assert parsed.info["flagged"] == 0 and parsed.info["records"] == 180


@pytest.mark.parametrize("size", [5000, 70000])
def test_long_lines(tmp_path, size):
    body = ("café \U0001f600 it's \\\"quoted\\\" \\u00e9\\ud83d\\ude00 back\\\\ " * (size // 50))
    long = ('{"user_id":"u","parent_asin":"p","rating":3.5,"text":"%s","title":"T"}' % body)
    assert len(long.encode()) >= size
    data = b"\n".join([b'{"user_id":"a","parent_asin":"p","rating":1}', long.encode(),
                       b'{"user_id":"b","parent_asin":"q","rating":2,"text":"after"}']) + b"\n"
    parsed = _check(tmp_path, data)
    assert parsed.info["flagged"] == 0 and parsed.info["records"] == 3


def test_neighbouring_lines_do_not_join(tmp_path):
    """A key one line lacks is not taken from its neighbour, and a string or a
    bracket left open (flagged) does not swallow the next line."""
    data = (b'{"user_id":"a","parent_asin":"p","rating":1}\n'
            b'{"user_id":"b","parent_asin":"q","text":"only here","helpful_vote":9}\n'
            b'{"user_id":"c","rating":5}\r'
            b'{"parent_asin":"r","rating":5,"timestamp":77,"verified_purchase":true}\n'
            b'{"user_id":"d","parent_asin":"s","rating":2}')
    parsed = _check(tmp_path, data)
    assert parsed.info["records"] == 2 and parsed.info["skipped"] == 3
    bad = b'{"user_id":"a","parent_asin":"p","rating":1,"text":"open\n{"user_id":"b","parent_asin":"q","rating":2}\n'
    with pytest.raises(ValueError):                          # json.JSONDecodeError, as the reader
        jsonl.read_reviews(bad)


@pytest.mark.parametrize("data", [b"", b"\n", b"\n\r\n  \n\t\n \r", b"   "])
def test_empty_and_blank_files(tmp_path, data):
    parsed = _check(tmp_path, data)
    assert len(parsed.cols) == 0 and len(parsed.user_ids) == 0 and len(parsed.item_ids) == 0
    assert parsed.info["records"] == 0 and parsed.info["blank"] == parsed.info["lines"]
    assert parsed.cols.rating.dtype == torch.float32 and parsed.cols.user.dtype == torch.int32


def test_input_already_on_the_device(plain, odd):
    for data, host in (plain, odd):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        _assert_equal(jsonl.read_reviews(t.cuda()), host)
        _assert_equal(jsonl.read_reviews(t.cuda(), chunk_bytes=700), host)
        _assert_equal(jsonl.read_reviews(t), host)
        _assert_equal(jsonl.read_reviews(np.frombuffer(data, np.uint8)), host)


@pytest.mark.parametrize("chunk_bytes", [1, 150, 1000])
def test_chunks_that_end_inside_lines(plain, odd, chunk_bytes):
    for data, host in (plain, odd):
        chunks = jsonl.plan_chunks(np.frombuffer(data, np.uint8), chunk_bytes)
        inside = [data[b0 + chunk_bytes - 1] not in b"\r\n" for b0, b1 in chunks[:-1]]
        assert sum(inside) > len(inside) // 2                 # the window's edge: inside a line
        parsed = jsonl.read_reviews(data, chunk_bytes=chunk_bytes)
        _assert_equal(parsed, host)
        assert parsed.info["chunks"] == len(chunks) > 3
        one = jsonl.read_reviews(data)
        assert {k: v for k, v in parsed.info.items() if k != "chunks"} == \
               {k: v for k, v in one.info.items() if k != "chunks"}


def test_a_too_long_line_is_refused(plain, monkeypatch):
    data, _ = plain
    longest = max(e - b for b, e in R.split_lines(data))
    monkeypatch.setattr(jsonl, "BYTES_MAX", longest + 2)     # line + terminator: one byte below
    assert len(jsonl.read_reviews(data, chunk_bytes=64).cols) > 0
    monkeypatch.setattr(jsonl, "BYTES_MAX", longest + 1)
    with pytest.raises(ValueError, match="line"):
        jsonl.read_reviews(data, chunk_bytes=64)


@pytest.mark.parametrize("line", R.ODD_RAISING)
def test_a_malformed_line_raises_what_the_reader_raises(tmp_path, line):
    data = b'{"user_id":"u","parent_asin":"p","rating":1}\n' + line + b"\n"
    with pytest.raises(Exception) as want:
        _host(tmp_path, data)
    with pytest.raises(Exception) as got:
        jsonl.read_reviews(data)
    assert type(got.value) is type(want.value), (got.value, want.value)


def _expected_fallback(data: bytes, mask: int) -> int:
    """The sides on which the device's rule meets two strings under one hash."""
    ref = R.parse(data, "parent_asin", jsonl.host_record)
    return sum(R.number_ids([ref[side + "_ids"][k] for k in ref[side].tolist()], mask)[2] > 0
               for side in ("user", "item"))


@pytest.mark.parametrize("mask", [0xFF, 0x3])
def test_a_narrow_hash_numbers_on_the_host(plain, mask):
    data, host = plain
    parsed = jsonl.read_reviews(data, _hash_mask=mask)
    _assert_equal(parsed, host)
    assert parsed.info["numbering_fallback"] == _expected_fallback(data, mask)
    if mask == 0x3:                                          # 19 users in 4 values must collide
        assert parsed.info["numbering_fallback"] == 2


def test_an_8_bit_hash_must_fall_back_on_300_ids(tmp_path):
    data = R.many_ids_corpus()
    parsed = jsonl.read_reviews(data, _hash_mask=0xFF)
    _assert_equal(parsed, _host(tmp_path, data))
    assert len(parsed.user_ids) == len(parsed.item_ids) == 300
    assert parsed.info["numbering_fallback"] == 2 == _expected_fallback(data, 0xFF)
    assert jsonl.read_reviews(data).info["numbering_fallback"] == 0


def test_numbering_at_sort_and_scan_sizes():
    """number_ids alone on 70,000 strings (several blocks of every kernel, runs
    longer than a wave): a few distinct ids far apart, and many distinct."""
    rng = np.random.default_rng(5)
    for pool in (37, 40_000):
        names = [b"id%d" % v * (1 + v % 3) for v in rng.integers(0, 10**9, pool)]
        pick = rng.integers(0, pool, 70_000)
        strings = [names[k] for k in pick.tolist()]
        seen: dict = {}
        want = np.fromiter((seen.setdefault(s, len(seen)) for s in strings), np.int32, len(strings))
        off = np.cumsum([0] + [len(s) for s in strings]).astype(np.int64)
        data = torch.frombuffer(bytearray(b"".join(strings)), dtype=torch.uint8).cuda()
        ids, table, fallback = jsonl.number_ids(data, torch.from_numpy(off).cuda())
        assert not fallback and ids.cpu().numpy().tobytes() == want.tobytes()
        assert _np(table.data).tobytes() == b"".join(seen)
        assert _np(table.offsets).tolist() == np.cumsum([0] + [len(s) for s in seen]).tolist()


def test_two_calls_give_the_same_bits(odd):
    data, _ = odd
    a, b = jsonl.read_reviews(data), jsonl.read_reviews(data)
    for name in COLUMNS:
        assert _np(getattr(a.cols, name)).tobytes() == _np(getattr(b.cols, name)).tobytes()
    assert torch.equal(a.cols.text.data, b.cols.text.data) and a.info == b.info
    assert torch.equal(a.user_ids.data, b.user_ids.data)


def _tensors(x) -> list:
    return [(k, v) for k, v in x._asdict().items() if isinstance(v, torch.Tensor)]


@pytest.mark.parametrize("feature_set", ["main", "v2"])
def test_end_to_end_graph(plain, feature_set):
    data, (cols, user2idx, item2idx) = plain
    parsed = jsonl.read_reviews(data)
    got = build_credibility_graph(parsed.cols, len(parsed.user_ids), len(parsed.item_ids),
                                  feature_set=feature_set)
    want = build_credibility_graph(cols, len(user2idx), len(item2idx), feature_set=feature_set)
    assert got.stats == want.stats or str(got.stats) == str(want.stats)
    for (k, a), (_, b) in zip(_tensors(got), _tensors(want)):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), k


def test_end_to_end_split(plain):
    from bbgr.split import IdTable
    data, (cols, user2idx, item2idx) = plain
    parsed = jsonl.read_reviews(data)
    got = split_interactions(parsed.cols.user, parsed.cols.item, parsed.cols.rating,
                             parsed.user_ids, parsed.item_ids)
    want = split_interactions(cols.user, cols.item, cols.rating,
                              IdTable(*(np.frombuffer(_table(user2idx)[0], np.uint8),
                                        _table(user2idx)[1])),
                              IdTable(*(np.frombuffer(_table(item2idx)[0], np.uint8),
                                        _table(item2idx)[1])))
    assert got.counts == want.counts and (got.num_users, got.num_items) == (want.num_users,
                                                                            want.num_items)
    assert sum(got.counts.values()) > 20
    for (k, a), (_, b) in zip(_tensors(got), _tensors(want)):
        assert torch.equal(a, b), k
