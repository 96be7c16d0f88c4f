"""CPU: the device's rule for review dumps, restated in tests/jsonl_ref.py,
against the host reader: every line the rule does not flag gives the reader's
record, every flagged line re-parsed by bbgr.jsonl.host_record does too, the
rule flags no line of the plain corpus, the numbering by hash equals the
reader's dicts (and reports collisions under a narrow mask), and the chunk
planner cuts at line ends."""
import json

import numpy as np
import pytest

import jsonl_ref as R
from bbgr import jsonl
from bbgr.features import review_columns_from_jsonl
from bbgr.split import id_table


def _reader(tmp_path, data: bytes, name="d.jsonl"):
    p = tmp_path / name
    p.write_bytes(data)
    return review_columns_from_jsonl(str(p), "parent_asin", tokens="host")


def _table_bytes(d: dict) -> list:
    return [s.encode("utf-8", "surrogatepass") for s in d]


def _texts(data: bytes) -> list:
    """The reader's text expression on the lines it keeps."""
    out = []
    for line in data.decode("utf-8", "replace").replace("\r\n", "\n").replace("\r", "\n").split("\n"):
        if not line.strip():
            continue
        r = json.loads(line)
        if r.get("rating") is None or not (r.get("user_id") and r.get("parent_asin")):
            continue
        out.append(" ".join((r.get("title") or "", r.get("text") or "")).encode("utf-8", "surrogatepass"))
    return out


def _same(tmp_path, data: bytes) -> dict:
    got = R.parse(data, "parent_asin", jsonl.host_record)
    cols, user2idx, item2idx = _reader(tmp_path, data)
    for name in ("user", "item", "rating", "helpful_vote", "verified", "timestamp", "ts_valid"):
        want = np.asarray(getattr(cols, name))
        assert got[name].dtype == want.dtype or name == "verified", name
        assert got[name].tobytes() == want.astype(got[name].dtype).tobytes(), name
    assert got["user_ids"] == _table_bytes(user2idx)
    assert got["item_ids"] == _table_bytes(item2idx)
    assert got["text"] == _texts(data)
    return got


def test_plain_corpus_is_exact_and_nothing_is_flagged(tmp_path):
    data = R.plain_corpus()
    got = _same(tmp_path, data)
    assert got["flagged"] == 0            # the GPU equality tests cannot hide behind the fallback
    assert got["records"] > 80 and got["skipped"] > 5
    assert len(got["user_ids"]) < got["records"] / 3


def test_odd_corpus_is_exact(tmp_path):
    data = R.odd_corpus()
    got = _same(tmp_path, data)
    assert got["flagged"] >= 20 and got["blank"] >= 6
    statuses = [R.scan_line(l, b"parent_asin")[0] for l in R.ODD_LINES]
    assert statuses[0] == R.FLAGGED                       # the key with a backslash
    assert statuses[4] == statuses[5] == R.KEPT           # 4.35, 5
    assert statuses[6] == R.FLAGGED and statuses[10] == R.KEPT and statuses[9] == R.FLAGGED
    assert R.scan_line(R.ODD_LAST, b"parent_asin")[0] == R.KEPT


@pytest.mark.parametrize("line", R.ODD_RAISING)
def test_lines_the_reader_refuses_are_flagged_and_raise_the_same(tmp_path, line):
    assert R.scan_line(line, b"parent_asin")[0] == R.FLAGGED
    with pytest.raises(Exception) as want:
        _reader(tmp_path, line + b"\n")
    with pytest.raises(Exception) as got:
        rec = jsonl.host_record(line, "parent_asin")
        np.asarray([rec[3]], np.int32)                     # the reader's conversion at its end
    assert type(got.value) is type(want.value)


def test_random_lines(tmp_path):
    lines = R.random_lines(2000)
    keep, kept, flagged, raising = [], 0, 0, 0
    for line in lines:
        status, rec = R.scan_line(line, b"parent_asin")
        try:
            host = jsonl.host_record(line, "parent_asin")
        except Exception:
            raising += 1
            assert status == R.FLAGGED, line               # never vouched for
            continue
        if status == R.FLAGGED:
            flagged += 1
        elif status == R.KEPT:
            kept += 1
            assert host not in (jsonl.BLANK, jsonl.SKIPPED), line
            assert rec[:2] == host[:2] and rec[7] == host[7], line
            assert np.float32(host[2]).tobytes() == rec[2].tobytes(), line
            assert rec[3:7] == host[3:7], line
        else:
            assert host == status, line
        if host in (jsonl.BLANK, jsonl.SKIPPED) or (-2**31 <= host[3] < 2**31
                                                    and -2**63 <= host[5] < 2**63):
            keep.append(line)
    assert kept > 300 and flagged > 300 and raising > 20, (kept, flagged, raising)
    _same(tmp_path, b"\n".join(keep) + b"\n")              # and against the reader itself


def test_numbering_by_hash_equals_first_appearance():
    got = R.parse(R.plain_corpus(), "parent_asin", jsonl.host_record)
    rng = np.random.default_rng(0)
    strings = [got["user_ids"][k] for k in rng.integers(0, len(got["user_ids"]), 400)]
    seen: dict = {}
    want = [seen.setdefault(s, len(seen)) for s in strings]
    ids, table, collisions = R.number_ids(strings)
    assert collisions == 0 and ids == want and table == list(seen)
    assert table == [bytes(id_table([s.decode()]).data) for s in seen]
    # 19 strings under 8 bits may or may not collide; under 2 bits they must
    assert R.number_ids(strings, 0x3)[2] > 0


def test_numbering_under_an_8_bit_mask_must_fall_back(tmp_path):
    """300 distinct ids a side cannot have 300 different 8-bit hashes: the rule
    reports collisions, where the wrapper numbers on the host; at full width it
    reports none and equals the reader's dicts."""
    data = R.many_ids_corpus()
    got = _same(tmp_path, data)
    for side, tab in (("user", got["user_ids"]), ("item", got["item_ids"])):
        assert len(tab) == 300
        strings = [tab[k] for k in got[side].tolist()]
        assert R.number_ids(strings, 0xFF)[2] > 0
        ids, table, collisions = R.number_ids(strings)
        assert collisions == 0 and table == tab and ids == got[side].tolist()


def test_line_rule():
    assert R.split_lines(b"a\nb\r\nc\rd") == [(0, 1), (2, 3), (4, 4), (5, 6), (7, 8)]
    assert R.split_lines(b"") == [] and R.split_lines(b"\n") == [(0, 0)]
    assert R.scan_line(b" \t", b"k")[0] == R.BLANK
    assert R.scan_line(b"\xc2\xa0", b"k")[0] == R.FLAGGED   # blank to str.strip() only


def test_chunk_planner(monkeypatch):
    data = np.frombuffer(b"ab\ncd\r\nefgh\nij", np.uint8)
    assert jsonl.plan_chunks(data, 4) == [(0, 3), (3, 7), (7, 12), (12, 14)]
    assert jsonl.plan_chunks(data, 1) == [(0, 3), (3, 6), (6, 7), (7, 12), (12, 14)]
    assert jsonl.plan_chunks(data, 100) == [(0, 14)]
    assert jsonl.plan_chunks(data[:0], 8) == []
    for cb in range(1, 16):
        ch = jsonl.plan_chunks(data, cb)
        assert ch[0][0] == 0 and ch[-1][1] == 14
        assert all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(data[b1 - 1] in (10, 13) for _, b1 in ch[:-1])
        assert all(b1 - b0 <= max(cb, 5) for b0, b1 in ch)
    with pytest.raises(ValueError):
        jsonl.plan_chunks(data, 0)
    monkeypatch.setattr(jsonl, "_SEARCH", 2)                # the search in steps
    assert jsonl.plan_chunks(data, 6) == [(0, 6), (6, 12), (12, 14)]
    monkeypatch.setattr(jsonl, "BYTES_MAX", 5)              # a line of BYTES_MAX bytes
    with pytest.raises(ValueError, match="line"):
        jsonl.plan_chunks(data, 4)
    assert jsonl.plan_chunks(data[:7], 4) == [(0, 3), (3, 7)]


@pytest.mark.parametrize("key", ["", 'a"b', "a\\b", "a\nb", "café", "k" * 256, 5])
def test_item_id_key_is_checked(key):
    with pytest.raises(ValueError):
        jsonl._key_bytes(key)
