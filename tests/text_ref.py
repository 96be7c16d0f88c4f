"""The token rule over UTF-8 bytes and the token hash of csrc/text.hip, in
plain Python: what the device counts, stated without a regex and without
``str.lower()``, plus the corpora the GPU tests run (so the CPU tests can show
that no two of their tokens share a full-width hash).

The rule: a letter is an ASCII A-Za-z (lower-cased) or the byte C4 directly
before B0 (U+0130 -> "i"; B0 separates); 0x27 is the apostrophe; all else and
the record's edges separate. A maximal letter run is attached when exactly one
apostrophe lies between it and the run before; a run begins a token unless it
is attached and the run before it began one, and then it is that token's
apostrophe part. U+212A (E2 84 AA, the Kelvin sign, lower() "k") is outside
the rule: ``has_kelvin`` says which records the device hands back.
"""
import random
import re

TEXT_STEP = 64
MASK64 = (1 << 64) - 1
KELVIN = b"\xe2\x84\xaa"
TOKEN = re.compile(r"[a-z]+(?:'[a-z]+)?")

# every phase of the rule: chains of apostrophe parts, a doubled apostrophe,
# a leading and a trailing one, U+0130, upper case
PATTERN = "ab'cd'ef'g X'y ''z İq 'r s'"


def regex_tokens(s: str) -> list:
    """main.py tokenize() / bbgr.features.tokenize."""
    return TOKEN.findall(s.lower()) if s else []


def _letter(bs: bytes, i: int) -> int:
    b = bs[i]
    if 65 <= b <= 90:
        return b + 32
    if 97 <= b <= 122:
        return b
    if b == 0xC4 and i + 1 < len(bs) and bs[i + 1] == 0xB0:
        return ord("i")
    return 0


def byte_tokens(bs: bytes) -> list:
    """The tokens of one record's bytes, as normalised byte strings."""
    runs = []                       # (start, end) of maximal letter runs
    i, n = 0, len(bs)
    while i < n:
        if _letter(bs, i):
            j = i
            while j < n and _letter(bs, j):
                j += 1
            runs.append((i, j))
            i = j
        else:
            i += 1
    toks, prev_began, prev_end = [], False, None
    for a, b in runs:
        word = bytes(_letter(bs, k) for k in range(a, b))
        attached = prev_end is not None and a == prev_end + 1 and bs[prev_end] == 0x27
        if attached and prev_began:
            toks[-1] = toks[-1] + b"'" + word
            prev_began = False
        else:
            toks.append(word)
            prev_began = True
        prev_end = b
    return toks


def has_kelvin(bs: bytes) -> bool:
    return KELVIN in bs


def token_hash(tok: bytes, mask: int = 0) -> int:
    """FNV-1a (64 bits) over the normalised bytes, a finaliser, the mask
    (0: all 64 bits)."""
    h = 0xCBF29CE484222325
    for c in tok:
        h = ((h ^ c) * 0x100000001B3) & MASK64
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & MASK64
    h ^= h >> 32
    return h & (mask or MASK64)


def counts(bs: bytes) -> tuple:
    toks = byte_tokens(bs)
    return len(toks), len(set(toks))


def collides(bs: bytes, mask: int = 0) -> bool:
    """Two distinct tokens of the record share a masked hash."""
    distinct = set(byte_tokens(bs))
    return len({token_hash(t, mask) for t in distinct}) < len(distinct)


def encode(s: str) -> bytes:
    return s.encode("utf-8", "surrogatepass")


# -- the corpora of tests/test_gpu_text.py ------------------------------------------------
def word(k: int) -> str:
    """The k-th word of an endless vocabulary of distinct lower-case words."""
    out = []
    k += 1
    while k:
        k, r = divmod(k - 1, 26)
        out.append(chr(97 + r))
    return "".join(out)


def sliding_records(pad: str) -> list:
    """PATTERN at every byte offset 0 .. 2 * TEXT_STEP + 40 of a record padded
    with `pad` on both sides."""
    return [pad * k + PATTERN + pad * 70 for k in range(2 * TEXT_STEP + 41)]


def length_records() -> list:
    """Records of the edge lengths, in letters and in a mix with apostrophes."""
    out = []
    for n in (0, 1, 2, TEXT_STEP - 1, TEXT_STEP, TEXT_STEP + 1, 2 * TEXT_STEP - 1,
              2 * TEXT_STEP + 1):
        out.append("a" * n)
        out.append(("b'c d" * n)[:n])
        out.append(("e " * n)[:n])
    return out


def count_records() -> list:
    """k tokens with 1, k / 2 and k distinct ones, for the listed k."""
    out = []
    for k in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097):
        for distinct in sorted({min(k, 1), k // 2, k}):
            out.append(" ".join(word(i % distinct) for i in range(k)) if distinct else "")
    return out


def unicode_records() -> list:
    return ["The the THE", "don't don t", "don't", "İ i I", "İstanbul istanbul", "\u212a k kelvin K \u212aelvin",
            "it’s it's its", "abc123def a_b _ 9", "a\x00b\x00'c", "x\U0001F600y \U0001F600'z",
            "ſ ß é straße", "i̇ i", "\ud83d lone 'q q' x''y", "rock'n'roll a'b'c'd'e",
            "\u212a", "a\u212a'b", "İ'İ İİ"]


def long_token_records() -> list:
    t = "q" * 2500 + "'" + "r" * 2499
    return [t + " " + t.upper(), t + " " + t[:-1] + "s", "z" * 5000 + " " + "Z" * 5000,
            "z" * 5000 + " " + "z" * 4999 + "y"]


def random_records(n: int, seed: int, max_tokens: int = 60) -> list:
    """Seeded review-like records: up to `max_tokens` words of a small
    vocabulary in mixed case, with punctuation, apostrophes and some
    non-ASCII."""
    rng = random.Random(seed)
    seps = [" ", " ", " ", ", ", ". ", "'", "''", " '", "' ", "-", "\n", " é ", " İ", "’", " 😀 "]
    out = []
    for _ in range(n):
        parts = []
        for _ in range(rng.randint(0, max_tokens)):
            w = word(rng.randint(0, 400))
            parts.append(rng.choice((w, w, w.upper(), w.capitalize())))
            parts.append(rng.choice(seps))
        out.append("".join(parts))
    return out


def neighbour_records() -> list:
    """Records whose edges cut a token: nothing joins across them."""
    return ["xx ab", "cd yy", "", "", "xx ab'", "cd", "", "xx ab", "'cd", "ab'", "", "'cd", "a",
            "'", "b", "İ"]


def all_corpora() -> dict:
    return {
        "sliding_dot": sliding_records("."), "sliding_a": sliding_records("a"),
        "lengths": length_records(), "counts": count_records(), "unicode": unicode_records(),
        "long": long_token_records(), "random": random_records(400, 11),
        "narrow": random_records(300, 12), "neighbours": neighbour_records(),
    }
