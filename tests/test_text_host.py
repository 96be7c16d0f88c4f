"""CPU: the byte rule of the device tokeniser (tests/text_ref.py) against the
reference's regex, the code points that make the rule complete, the record
table and the chunk planner of bbgr.text, and the full-width hash on every
corpus the GPU tests run."""
import random
import sys

import numpy as np
import pytest

import text_ref as TR
from bbgr import text as T
from bbgr.features import ReviewColumns, build_credibility_graph, tokenize

FIXED = [
    "", " ", "'", "''", "a", "A", "a'", "'a", "a'b", "a''b", "a'b'c", "a'b'c'd'e", "rock'n'roll",
    "x''y 'q q'", "The the THE", "don't don t", "İ", "İstanbul \u212aELVİN", "İ'İ",
    "aİb", "i̇", "K", "\u212a", "a\u212a'b",
    "’", "it’s", "ſ ß é", "a\x00b", "abc123def a_b", "x\U0001F600y", TR.PATTERN,
    "a" * 200 + "'" + "b" * 200 + "'" + "c",
]
ALPHABET = ["a", "b", "Z", "'", "'", " ", "1", "_", "İ", "K", "é", "̇", "’", "\U0001F600",
            "ſ", "ß", "\x00", "I", "\u212a"]


def _strip_kelvin(s: str) -> str:
    """The rule leaves U+212A to the host: compare on strings without it."""
    return s.replace("\u212a", "")


@pytest.mark.parametrize("s", FIXED)
def test_byte_rule_equals_the_regex_on_fixed_strings(s):
    if "\u212a" in s:
        assert TR.has_kelvin(TR.encode(s))
        s = _strip_kelvin(s)
    assert [t.decode() for t in TR.byte_tokens(TR.encode(s))] == tokenize(s) == TR.regex_tokens(s)


def test_byte_rule_equals_the_regex_on_random_strings():
    rng = random.Random(1)
    kelvin = 0
    for _ in range(20000):
        s = "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 14)))
        bs = TR.encode(s)
        assert TR.has_kelvin(bs) == ("\u212a" in s)
        if TR.has_kelvin(bs):
            kelvin += 1
            s = _strip_kelvin(s)
            bs = TR.encode(s)
        assert [t.decode() for t in TR.byte_tokens(bs)] == tokenize(s), repr(s)
    assert kelvin > 1000


def test_only_two_code_points_outside_ascii_lower_into_the_token_alphabet():
    """A Python whose Unicode tables add a third fails here: the byte rule
    would then miss a letter."""
    wanted = set("abcdefghijklmnopqrstuvwxyz'")
    found = [cp for cp in range(0x80, sys.maxunicode + 1) if wanted & set(chr(cp).lower())]
    assert found == [0x130, 0x212A]
    assert "İ".lower() == "i̇" and "\u212a".lower() == "k"
    assert TR.encode("İ") == b"\xc4\xb0" and TR.encode("\u212a") == TR.KELVIN
    # and inside ASCII, lower() is the rule's own folding
    for cp in range(0x80):
        low = chr(cp).lower()
        assert low == (chr(cp + 32) if 65 <= cp <= 90 else chr(cp))


def test_every_corpus_of_the_gpu_tests_follows_the_regex():
    for name, records in TR.all_corpora().items():
        for s in records:
            if "\u212a" in s:
                continue
            toks = tokenize(s)
            assert TR.counts(TR.encode(s)) == (len(toks), len(set(toks))), (name, s[:40])


def test_no_two_tokens_of_the_gpu_corpora_share_a_full_width_hash():
    """So the GPU tests' zero-recheck condition holds by the reference alone."""
    seen = {}
    for records in TR.all_corpora().values():
        for s in records:
            for tok in TR.byte_tokens(TR.encode(s)):
                assert seen.setdefault(TR.token_hash(tok), tok) == tok
    assert len(seen) > 4000
    # the narrow mask does collide: the 0xFF tests have something to find
    narrow = [TR.collides(TR.encode(s), 0xFF) for s in TR.all_corpora()["narrow"]]
    assert 20 < sum(narrow) < len(narrow) - 20


def test_from_strings_offsets():
    strings = ["ab", "", "İ", "\ud83d", "x\U0001F600"]
    t = T.ReviewText.from_strings(strings)
    assert len(t) == 5 and t.offsets.dtype == np.int64 and t.data.dtype == np.uint8
    assert t.offsets.tolist() == [0, 2, 2, 4, 7, 12]
    assert t.data.tobytes() == b"ab\xc4\xb0\xed\xa0\xbdx\xf0\x9f\x98\x80"
    empty = T.ReviewText.from_strings([])
    assert len(empty) == 0 and empty.offsets.tolist() == [0] and empty.data.shape == (0,)
    with pytest.raises(UnicodeEncodeError):
        "\ud83d".encode("utf-8")          # why surrogatepass
    assert T.host_counts(TR.encode("\ud83d a'b A'B K")) == (3, 2)


def test_chunk_planner():
    off = np.array([0, 10, 10, 25, 40, 1040, 1045, 1045], np.int64)
    # a record longer than chunk_bytes is a chunk of its own
    assert T.plan_chunks(off, 30) == [(0, 3), (3, 4), (4, 5), (5, 7)]
    assert T.plan_chunks(off, 1 << 30) == [(0, 7)]
    assert T.plan_chunks(off, 1) == [(r, r + 1) for r in range(7)]
    for cb in (1, 7, 15, 30, 1000, 1045):
        chunks = T.plan_chunks(off, cb)
        assert chunks[0][0] == 0 and chunks[-1][1] == 7
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for r0, r1 in chunks:
            assert r1 > r0 and (off[r1] - off[r0] <= cb or r1 == r0 + 1)
    assert T.plan_chunks(np.zeros(1, np.int64), 100) == []
    assert T.plan_chunks(np.zeros(6, np.int64), 100) == [(0, 5)]      # all empty, n > 0
    assert T.plan_chunks(np.array([5, 9, 20], np.int64), 11) == [(0, 1), (1, 2)]
    # below 2^31 - 1 bytes whatever chunk_bytes says
    big = np.array([0, 2**31 - 2, 2**31 + 5], np.int64)
    assert T.plan_chunks(big, 1 << 40) == [(0, 1), (1, 2)]
    with pytest.raises(ValueError, match="record 1 has"):
        T.plan_chunks(np.array([0, 4, 4 + 2**31 - 1], np.int64), 1 << 30)
    with pytest.raises(ValueError, match="chunk_bytes"):
        T.plan_chunks(off, 0)


def test_a_too_long_record_is_refused_before_any_launch():
    zeros = np.zeros(2**31 - 1, np.uint8)    # untouched pages: nothing is written or copied
    with pytest.raises(ValueError, match="record 0 has 2147483647 bytes"):
        T.token_counts(T.ReviewText(zeros, np.array([0, 2**31 - 1], np.int64)))
    with pytest.raises(ValueError, match="outside the 8 bytes"):
        T.token_counts(T.ReviewText(zeros[:8], np.array([0, 9], np.int64)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        T.token_counts(T.ReviewText.from_strings(["a"]), device="cpu")


def test_review_columns_defaults_and_missing_token_columns():
    z = np.zeros(3, np.int32)
    cols = ReviewColumns(z, z, z.astype(np.float32), z, z.astype(np.uint8), z.astype(np.int64))
    assert cols.n_tokens is None and cols.n_unique_tokens is None and cols.text is None
    # positional order is unchanged: ts_valid is still the ninth
    cols9 = ReviewColumns(z, z, z, z, z, z, z + 1, z + 2, z + 3)
    assert cols9.n_tokens[0] == 1 and cols9.n_unique_tokens[0] == 2 and cols9.ts_valid[0] == 3
    with pytest.raises(ValueError, match="n_tokens / n_unique_tokens"):
        build_credibility_graph(cols, 1, 1, "cuda")
    cols.text = T.ReviewText.from_strings(["a", "b"])
    with pytest.raises(ValueError, match="text: expected 3 records, got 2"):
        build_credibility_graph(cols, 1, 1, "cuda")
