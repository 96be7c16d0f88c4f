"""GPU: token and distinct-token counts of review text on the device
(bbgr_text_count, bbgr_text_unique, bbgr.text) against bbgr.features.tokenize.
Every comparison is integer equality. The corpora live in tests/text_ref.py;
tests/test_text_host.py shows on the CPU that no two of their tokens share a
full-width hash, so with hash_mask = 0 the device must vouch for every record
free of U+212A."""
import dataclasses
import functools
import json

import numpy as np
import pytest
import torch

import text_ref as TR
from bbgr import text as T
from bbgr.features import build_credibility_graph, review_columns_from_jsonl, tokenize

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A
GUARD = 96
KELVIN = "\u212a"


@functools.lru_cache(maxsize=None)
def _corpus(name: str) -> tuple:
    return tuple(TR.all_corpora()[name])


@functools.lru_cache(maxsize=None)
def _expected(name: str):
    """(n_tokens, n_unique_tokens, holds U+212A) per record by the reference's regex."""
    toks = [tokenize(s) for s in _corpus(name)]
    return (np.array([len(t) for t in toks], np.int32),
            np.array([len(set(t)) for t in toks], np.int32),
            np.array([KELVIN in s for s in _corpus(name)], bool))


def _want(strings):
    toks = [tokenize(s) for s in strings]
    return [len(t) for t in toks], [len(set(t)) for t in toks]


def _launch(records, mask=0, lead=b"", tail=b""):
    """The two C calls on `records` (bytes) laid back to back after `lead` and
    before `tail`; the outputs are leading views of sentinel-filled buffers,
    and the GUARD elements behind each must come back untouched. Returns
    (n_tokens, n_unique_tokens, recheck, tokens, flagged) as numpy / ints."""
    n = len(records)
    blob = lead + b"".join(records) + tail
    off = np.zeros(n + 1, np.int64)
    off[0] = len(lead)
    if n:
        off[1:] = len(lead) + np.cumsum([len(r) for r in records])
    data = torch.from_numpy(np.frombuffer(blob + b"\0", np.uint8).copy()).to(DEV)
    n_tok = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    n_uniq = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    recheck = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    totals = torch.full((2 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    tokens, flagged = T._run_chunk(data, torch.from_numpy(off).to(DEV), int(off[0]), int(off[-1]),
                                   mask, n_tok[:n], n_uniq[:n], recheck[:n], totals[:2])
    torch.cuda.synchronize()
    for name, buf, used in (("n_tokens", n_tok, n), ("n_unique_tokens", n_uniq, n),
                            ("recheck", recheck, n), ("totals", totals, 2)):
        assert bool((buf[used:] == SENTINEL).all()), f"{name}: written past its {used} entries"
    return (n_tok[:n].cpu().numpy(), n_uniq[:n].cpu().numpy(), recheck[:n].cpu().numpy(), tokens,
            flagged)


def _check_strings(strings, **kw):
    """Full-width hash: exact on every record free of U+212A, none of them
    flagged; every record that holds it flagged."""
    nt, nu, rc, tokens, flagged = _launch([TR.encode(s) for s in strings], **kw)
    want_t, want_u = _want(strings)
    kelvin = np.array([KELVIN in s for s in strings], bool)
    assert rc.tolist() == kelvin.astype(np.uint8).tolist()
    assert flagged == int(kelvin.sum()) and tokens == int(nt.sum())
    ok = ~kelvin
    assert nt[ok].tolist() == np.array(want_t, np.int32)[ok].tolist()
    assert nu[ok].tolist() == np.array(want_u, np.int32)[ok].tolist()
    return nt, nu, rc


@pytest.mark.parametrize("name", ["sliding_dot", "sliding_a", "lengths", "counts", "unicode",
                                  "long", "random", "neighbours"])
def test_corpus_full_width_hash(name):
    """sliding_*: the pattern of every phase at every byte offset 0 .. 2 *
    TEXT_STEP + 40, padded with '.' and with the letter 'a' (one token over
    several steps). lengths: 0, 1, 2, TEXT_STEP - 1 .. 2 * TEXT_STEP + 1.
    counts: 0 .. 4097 tokens a record with 1, k / 2, k distinct. long: a
    5,000-letter token twice in different case (1 distinct) and with its last
    letter changed (2). neighbours: tokens cut by record edges."""
    assert T.TEXT_STEP == TR.TEXT_STEP
    nt, nu, rc = _check_strings(list(_corpus(name)))
    want_t, want_u, kelvin = _expected(name)
    assert nt[~kelvin].tolist() == want_t[~kelvin].tolist()
    assert nu[~kelvin].tolist() == want_u[~kelvin].tolist()


def test_the_named_cases():
    """Case folding, the apostrophe part, U+0130 as i, and what separates."""
    cases = {
        "The the THE": (3, 1), "don't don t": (3, 3), "İ i": (2, 1), "İstanbul istanbul": (3, 3),
        "it’s": (2, 2), "abc123def a_b": (4, 4), "a\x00b": (2, 2), "x\U0001F600y": (2, 2),
        "rock'n'roll": (2, 2), "a'b'c'd'e": (3, 3), "x''y": (2, 2), "'q": (1, 1), "q'": (1, 1),
        "a'b A'B a b": (4, 3), "z" * 5000 + " " + "Z" * 5000: (2, 1),
        "z" * 5000 + " " + "z" * 4999 + "y": (2, 2),
    }
    assert {s: tuple(_want([s])[k][0] for k in (0, 1)) for s in cases} == cases
    nt, nu, _ = _check_strings(list(cases))
    assert list(zip(nt.tolist(), nu.tolist())) == list(cases.values())


@pytest.mark.parametrize("shift", range(16))
def test_record_starts_at_every_alignment(shift):
    strings = [TR.PATTERN, "a" * (TR.TEXT_STEP + shift), "b'c " * 40, "", "Zz zz'q"]
    _check_strings(strings, lead=b"." * shift)


def test_letters_outside_the_range_are_not_read_as_text():
    """offsets[0] > 0; letters lie directly before offsets[0] and after offsets[n]."""
    strings = ["cd ef", "", "gh'", "ij"]
    for lead, tail in ((b"ab", b"kl"), (b"ab'", b"'kl"), (b"x" * 70, b"y" * 70), (b"\xc4", b"\xb0")):
        _check_strings(strings, lead=lead, tail=tail)
    # the last byte of the range is C4 and B0 follows it outside: not a letter
    nt, nu, rc, _, _ = _launch([b"a \xc4"], tail=b"\xb0b")
    assert (nt.tolist(), nu.tolist(), rc.tolist()) == ([1], [1], [0])


def test_neighbouring_records_do_not_join():
    for left, right, want in (("xx ab", "cd yy", (2, 2)), ("xx ab'", "cd", (2, 1)),
                              ("xx ab", "'cd", (2, 1))):
        strings = [left, "", "", right, ""]
        nt, nu, _ = _check_strings(strings)
        assert (nt[0], nt[3]) == want and nt[1] == nt[2] == nt[4] == 0
    # U+0130 cut between two records: C4 ends one (no B0 follows inside it)
    nt, nu, rc, _, _ = _launch([b"a\xc4", b"\xb0b", b"\xc4\xb0"])
    assert nt.tolist() == [TR.counts(r)[0] for r in (b"a\xc4", b"\xb0b", b"\xc4\xb0")] == [1, 1, 1]
    assert nu.tolist() == [1, 1, 1] and rc.tolist() == [0, 0, 0]
    # U+212A cut between two records is no U+212A
    nt, nu, rc, _, _ = _launch([b"a\xe2\x84", b"\xaab", b"\xe2", b"\x84\xaa"])
    assert rc.tolist() == [0, 0, 0, 0] and nt.tolist() == [1, 1, 0, 0]


def test_one_letter_records_back_to_back():
    """A record's edge separates without a byte: as many tokens as bytes."""
    words = [TR.word(k % 26) for k in range(5000)]          # "a" .. "z", 5,000 bytes, 5,000 tokens
    nt, nu, rc, tokens, flagged = _launch([w.encode() for w in words])
    assert nt.tolist() == [1] * 5000 and nu.tolist() == [1] * 5000
    assert tokens == 5000 and flagged == 0 and not rc.any()
    a, b, info = T.token_counts(T.ReviewText.from_strings(["a", "b", "c"]))
    assert a.tolist() == [1, 1, 1] and b.tolist() == [1, 1, 1] and info["tokens"] == 3
    strings = ["a b", "c", "", "d'e", "f"] * 1000             # 2 tokens in 3 bytes, over and over
    want_t, want_u = _want(strings)
    for chunk_bytes in (1 << 30, 64, 3):
        a, b, info = T.token_counts(T.ReviewText.from_strings(strings), chunk_bytes=chunk_bytes)
        assert a.tolist() == want_t and b.tolist() == want_u and info["tokens"] == sum(want_t)


def test_text_already_on_the_device():
    strings = list(_corpus("unicode") + _corpus("neighbours") + _corpus("random")[:50])
    host = T.ReviewText.from_strings(strings)
    there = T.ReviewText(torch.from_numpy(host.data.copy()).to(DEV),
                         torch.from_numpy(host.offsets).to(DEV))
    want_t, want_u = _want(strings)
    for text, chunk_bytes in ((there, 1 << 30), (there, 300),
                              (T.ReviewText(torch.from_numpy(host.data.copy()), host.offsets), 300)):
        a, b, info = T.token_counts(text, chunk_bytes=chunk_bytes)
        assert a.tolist() == want_t and b.tolist() == want_u
        assert info["rechecked"] == sum(KELVIN in s for s in strings) > 0


def test_kelvin_is_flagged_at_every_step_phase():
    """E2 84 AA at every offset around the step edges: flagged there and only there."""
    strings = ["." * k + KELVIN + "elvin k" for k in range(2 * TR.TEXT_STEP + 3)]
    strings += ["." * k + "\u2129" + "elvin k" for k in (0, 61, 62, 63, 64)]   # E2 84 A9
    _check_strings(strings)


def test_all_empty_input_and_no_records():
    nt, nu, rc, tokens, flagged = _launch([b""] * 300)
    assert not nt.any() and not nu.any() and not rc.any() and tokens == 0 and flagged == 0
    a, b, info = T.token_counts(T.ReviewText.from_strings([]))
    assert a.numel() == 0 and b.numel() == 0 and info == {"tokens": 0, "rechecked": 0, "chunks": 0}
    a, b, info = T.token_counts(T.ReviewText.from_strings(["", "", ""]))
    assert a.tolist() == [0, 0, 0] and b.tolist() == [0, 0, 0] and info["chunks"] == 1


def test_two_calls_give_the_same_bits():
    for mask in (0, 0xFF):
        records = [TR.encode(s) for s in _corpus("narrow") + _corpus("unicode")]
        one, two = _launch(records, mask=mask), _launch(records, mask=mask)
        for a, b in zip(one[:3], two[:3]):
            assert a.tobytes() == b.tobytes()
        assert one[3:] == two[3:]


def test_narrow_hash_flags_every_collision_and_stays_exact():
    strings = list(_corpus("narrow"))
    records = [TR.encode(s) for s in strings]
    want_t, want_u, _ = _expected("narrow")
    assert int(want_u.max()) <= 60
    nt, nu, rc, tokens, flagged = _launch(records, mask=0xFF)
    assert nt.tolist() == want_t.tolist() and tokens == int(want_t.sum())
    clear = rc == 0
    assert nu[clear].tolist() == want_u[clear].tolist()
    collide = np.array([TR.collides(r, 0xFF) for r in records], bool)
    assert collide.any() and (~collide).any()
    assert bool(rc[collide].all()), "a record with two tokens of equal masked hash went unflagged"
    assert flagged == int(rc.sum())
    # the wrapper counts the flagged ones again on the host
    a, b, info = T.token_counts(T.ReviewText.from_strings(strings), _hash_mask=0xFF)
    assert a.cpu().numpy().tolist() == want_t.tolist()
    assert b.cpu().numpy().tolist() == want_u.tolist()
    assert info["rechecked"] == flagged > 0 and info["tokens"] == int(want_t.sum())


def test_token_counts_is_exact_with_kelvin_and_in_chunks():
    strings = list(_corpus("random") + _corpus("unicode") + _corpus("neighbours"))
    text = T.ReviewText.from_strings(strings)
    assert 40_000 < text.data.shape[0] < 200_000
    want_t, want_u = _want(strings)
    a, b, info = T.token_counts(text)
    assert a.dtype == b.dtype == torch.int32 and a.is_cuda
    assert a.tolist() == want_t and b.tolist() == want_u
    assert info == {"tokens": sum(want_t), "rechecked": sum(KELVIN in s for s in strings),
                    "chunks": 1}
    a2, b2, info2 = T.token_counts(text, chunk_bytes=1000)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    assert info2["chunks"] > 40 and {k: info2[k] for k in ("tokens", "rechecked")} == \
        {k: info[k] for k in ("tokens", "rechecked")}
    # a record longer than chunk_bytes is a chunk of its own
    a3, b3, _ = T.token_counts(text, chunk_bytes=50)
    assert torch.equal(a, a3) and torch.equal(b, b3)


def _write_jsonl(path):
    rng = np.random.default_rng(5)
    texts = list(_corpus("random"))
    extra = ["KKelvin K", "İstanbul İ", "lone \ud83d surrogate's", "", None]
    with open(path, "w", encoding="utf-8") as f:
        for k in range(300):
            r = {"user_id": f"u{int(rng.integers(40))}", "parent_asin": f"i{int(rng.integers(25))}",
                 "rating": float(rng.integers(1, 6)), "helpful_vote": int(rng.integers(0, 9)),
                 "verified_purchase": bool(rng.integers(2)),
                 "timestamp": 1_600_000_000_000 + int(rng.integers(0, 10**10))}
            title, text = texts[k], extra[(k // 3 + 1) % len(extra)] if k % 3 == 0 else texts[399 - k]
            if k % 7 != 0:
                r["title"] = title if k % 11 else None
            if k % 5 != 0:
                r["text"] = text
            if k % 50 == 49:
                r.pop("rating")        # a skipped record
            f.write(json.dumps(r) + "\n")        # ensure_ascii: K, İ, \ud83d as escapes


def test_jsonl_end_to_end(tmp_path):
    path = tmp_path / "reviews.jsonl"
    _write_jsonl(path)
    raw = path.read_text()
    assert "\\u212a" in raw and "\\u0130" in raw and "\\ud83d" in raw and '"title": null' in raw
    host, u_h, i_h = review_columns_from_jsonl(path)
    dev, u_d, i_d = review_columns_from_jsonl(path, tokens="device")
    assert u_h == u_d and i_h == i_d and len(host) == len(dev) == 294
    assert host.text is None and len(dev.text) == len(dev)
    for f in dataclasses.fields(host):
        if f.name == "text":
            continue
        a, b = getattr(host, f.name), getattr(dev, f.name)
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
        assert a.dtype == b.dtype and a.tolist() == b.tolist(), f.name
    assert int(host.n_tokens.max()) > 50 and int((host.n_tokens == 0).sum()) > 0
    # the build from the text alone against the build from the two columns
    g_cols = build_credibility_graph(host, len(u_h), len(i_h), DEV)
    from_text = dataclasses.replace(host, n_tokens=None, n_unique_tokens=None, text=dev.text)
    g_text = build_credibility_graph(from_text, len(u_h), len(i_h), DEV)
    for name in ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
                 "helpful_reviews"):
        a, b = getattr(g_cols, name).cpu().numpy(), getattr(g_text, name).cpu().numpy()
        assert a.tobytes() == b.tobytes(), name
    assert g_cols.stats == g_text.stats
    with pytest.raises(ValueError, match="'host' or 'device'"):
        review_columns_from_jsonl(path, tokens="gpu")
