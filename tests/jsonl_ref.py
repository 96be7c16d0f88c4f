"""Host restatement of the device's rule for review dumps (csrc/jsonl.hip,
include/bbgr.h) over bytes: lines, the string mask and bracket depth, the key
search, what is vouched for, unescaping, and the numbering by hash, sort and
comparison; and the corpora the tests of bbgr.jsonl share."""
import json
import random
import re

import numpy as np

BLANK, SKIPPED, KEPT, FLAGGED = 0, 1, 2, 3
KEYS = [b"user_id", None, b"rating", b"helpful_vote", b"verified_purchase", b"timestamp",
        b"title", b"text"]
_BLANKS = (0x20, 0x09)
_NUMBER = re.compile(rb"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?")


def split_lines(data: bytes) -> list:
    """[(beg, end), ..]: '\\n' and '\\r' both end a line; a last line without a
    terminator counts."""
    out, beg = [], 0
    for p, b in enumerate(data):
        if b in (10, 13):
            out.append((beg, p))
            beg = p + 1
    if beg < len(data):
        out.append((beg, len(data)))
    return out


def _utf8(cp: int) -> bytes:
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | cp >> 6, 0x80 | cp & 0x3F])
    if cp < 0x10000:
        return bytes([0xE0 | cp >> 12, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F])
    return bytes([0xF0 | cp >> 18, 0x80 | cp >> 12 & 0x3F, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F])


def _hex4(d: bytes, i: int):
    h = d[i:i + 4]
    return int(h, 16) if len(h) == 4 and re.fullmatch(rb"[0-9a-fA-F]{4}", h) else None


_ESC = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10,
        ord("r"): 13, ord("t"): 9}


def unescape(d: bytes, q: int):
    """The string whose opening quote is d[q]: (its bytes, the position behind
    its closing quote), or None when the device does not vouch for it."""
    i, out, end = q + 1, bytearray(), len(d)
    while True:
        if i >= end:
            return None
        c = d[i]
        if c == 0x22:
            return bytes(out), i + 1
        if c < 0x20:
            return None
        if c == 0x5C:
            if i + 1 >= end:
                return None
            e = d[i + 1]
            i += 2
            if e == ord("u"):
                cp = _hex4(d, i)
                if cp is None:
                    return None
                i += 4
                if 0xD800 <= cp < 0xDC00 and i + 6 <= end and d[i:i + 2] == b"\\u":
                    lo = _hex4(d, i + 2)
                    if lo is None:
                        return None
                    if 0xDC00 <= lo < 0xE000:
                        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00)
                        i += 6
                out += _utf8(cp)
                continue
            if e not in _ESC:
                return None
            out.append(_ESC[e])
            continue
        if c < 0x80:
            out.append(c)
            i += 1
            continue
        lo, hi = 0x80, 0xBF
        if 0xC2 <= c <= 0xDF:
            n = 1
        elif c == 0xE0:
            n, lo = 2, 0xA0
        elif c == 0xED:
            n, hi = 2, 0x9F
        elif 0xE1 <= c <= 0xEF:
            n = 2
        elif c == 0xF0:
            n, lo = 3, 0x90
        elif 0xF1 <= c <= 0xF3:
            n = 3
        elif c == 0xF4:
            n, hi = 3, 0x8F
        else:
            return None
        if i + n >= end or not lo <= d[i + 1] <= hi:
            return None
        if any(d[i + k] & 0xC0 != 0x80 for k in range(2, n + 1)):
            return None
        out += d[i:i + n + 1]
        i += n + 1


def ends(d: bytes, i: int) -> bool:
    """A value ends at a blank, ',' or '}' inside the line."""
    return i < len(d) and d[i] in (0x20, 0x09, 0x2C, 0x7D)


def number(d: bytes, q: int):
    """(neg, digits, n_digits, frac) of the literal at d[q] (frac -1: no
    point), or None when it is not of the vouched form or does not end at a
    blank, ',' or '}' inside the line."""
    m = _NUMBER.match(d, q)
    if not m:
        return None
    frac = m.group(3)
    digits = m.group(2) + (frac or b"")
    if len(digits) > 18:
        return None
    if not ends(d, m.end()):
        return None
    return m.group(1) == b"-", int(digits), len(digits), -1 if frac is None else len(frac)


def scan_line(line: bytes, item_key: bytes):
    """(status, record): record = (user id, item id, rating float32,
    helpful_vote, verified, timestamp, ts_valid, text) for a KEPT line."""
    keys = [item_key if k is None else k for k in KEYS]
    flag = esc = in_str = closed = seen = False
    depth = 0
    vp = [-1] * 8
    n = len(line)
    for p, b in enumerate(line):
        escaped, esc = esc, (b == 0x5C and not esc)
        quote = b == 0x22 and not escaped
        if quote:
            in_str = not in_str
        out = not quote and not in_str
        if (b < 0x20 and not (out and b == 9)) or (out and b == 0x5C):
            flag = True
        nonblank = b not in _BLANKS
        if not seen and nonblank:
            seen = True
            flag |= b != 0x7B
        closer = out and b in (0x7D, 0x5D)
        if closed:
            flag |= nonblank
        elif closer and depth == 1:
            flag |= b != 0x7D
            closed = True
        if out and b == 0x3A and depth == 1:
            q = p - 1
            while q >= 0 and line[q] in _BLANKS:
                q -= 1
            if q < 0 or line[q] != 0x22:
                flag = True
            else:
                kend = q
                q -= 1
                bad = False
                while q >= 0 and line[q] != 0x22:
                    bad |= line[q] == 0x5C
                    q -= 1
                if q < 0 or (q > 0 and line[q - 1] == 0x5C):
                    bad = True
                if bad:
                    flag = True
                else:
                    v = p + 1
                    while v < n and line[v] in _BLANKS:
                        v += 1
                    for s in range(8):
                        if line[q + 1:kend] == keys[s]:
                            vp[s] = v
        if out and b in (0x7B, 0x5B):
            depth += 1
        elif closer:
            depth -= 1
    if not seen:
        return BLANK, None
    if flag or in_str or depth != 0 or not closed:
        return FLAGGED, None
    vals, absent = [None] * 8, [True] * 8
    for s in range(8):
        q = vp[s]
        if q < 0:
            continue
        if q >= n:
            return FLAGGED, None
        if line[q] == ord("n"):
            if line[q:q + 4] != b"null" or not ends(line, q + 4):
                return FLAGGED, None
            continue
        if s in (0, 1, 6, 7):
            v = unescape(line, q) if line[q] == 0x22 else None
            if v is None or not ends(line, v[1]):
                return FLAGGED, None
            v = v[0]
            if not v and s < 2:
                continue
            vals[s], absent[s] = v, False
        elif s == 4:
            if line[q:q + 4] == b"true" and ends(line, q + 4):
                vals[s] = True
            elif line[q:q + 5] == b"false" and ends(line, q + 5):
                vals[s] = False
            else:
                return FLAGGED, None
            absent[s] = False
        else:
            num = number(line, q)
            if num is None:
                return FLAGGED, None
            neg, digits, nd, frac = num
            if s == 2:
                if nd > 15 or (neg and digits == 0):
                    return FLAGGED, None
                x = digits / 10 ** frac if frac > 0 else float(digits)
                vals[s] = np.float32(-x if neg else x)
            else:
                if frac >= 0:
                    return FLAGGED, None
                x = -digits if neg else digits
                if s == 3 and not -2**31 <= x < 2**31:
                    return FLAGGED, None
                vals[s] = x
            absent[s] = False
    if absent[0] or absent[1] or absent[2]:
        return SKIPPED, None
    return KEPT, (vals[0], vals[1], vals[2], vals[3] or 0, bool(vals[4]), vals[5] or 0,
                  not absent[5], (vals[6] or b"") + b" " + (vals[7] or b""))


def string_hash(s: bytes, mask: int) -> int:
    h = 0xcbf29ce484222325
    for b in s:
        h = ((h ^ b) * 0x100000001b3) & (2**64 - 1)
    h ^= h >> 29
    h = (h * 0xbf58476d1ce4e5b9) & (2**64 - 1)
    h ^= h >> 32
    return h & (mask or 2**64 - 1)


def number_ids(strings: list, mask: int = 0):
    """(ids, table, collisions): the device's numbering: a stable sort by hash,
    run heads where the hash changes, a comparison with the left neighbour
    inside a run, ids in order of the heads' records. With collisions the ids
    are not vouched for."""
    n = len(strings)
    order = sorted(range(n), key=lambda r: string_hash(strings[r], mask))
    hashes = [string_hash(strings[r], mask) for r in order]
    collisions, run_head, heads = 0, {}, []
    for j, r in enumerate(order):
        if j == 0 or hashes[j] != hashes[j - 1]:
            heads.append(r)
            head = r
        elif strings[r] != strings[order[j - 1]]:
            collisions += 1
        run_head[r] = head
    rank = {r: k for k, r in enumerate(sorted(heads))}
    return [rank[run_head[r]] for r in range(n)], [strings[r] for r in sorted(heads)], collisions


def parse(data: bytes, item_id_key: str = "parent_asin", fallback=None) -> dict:
    """The whole rule: per line ``scan_line``; a flagged line goes to
    ``fallback(line bytes, item_id_key)`` (bbgr.jsonl.host_record). Columns as
    the reader types them, ids numbered by first appearance."""
    key = item_id_key.encode("ascii")
    recs, counts = [], {"lines": 0, "blank": 0, "skipped": 0, "flagged": 0}
    for beg, end in split_lines(data):
        counts["lines"] += 1
        status, rec = scan_line(data[beg:end], key)
        if status == FLAGGED:
            counts["flagged"] += 1
            rec = fallback(data[beg:end], item_id_key)
            status = rec if rec in (BLANK, SKIPPED) else KEPT
        if status == KEPT:
            recs.append(rec)
        else:
            counts["blank" if status == BLANK else "skipped"] += 1
    user, user_tab, _ = number_ids([r[0] for r in recs])
    item, item_tab, _ = number_ids([r[1] for r in recs])
    return dict(
        user=np.asarray(user, np.int32), item=np.asarray(item, np.int32),
        rating=np.asarray([r[2] for r in recs], np.float32),
        helpful_vote=np.asarray([r[3] for r in recs], np.int32),
        verified=np.asarray([r[4] for r in recs], np.uint8),
        timestamp=np.asarray([r[5] for r in recs], np.int64),
        ts_valid=np.asarray([r[6] for r in recs], np.bool_),
        text=[r[7] for r in recs], user_ids=user_tab, item_ids=item_tab,
        records=len(recs), **counts)


# -- corpora ---------------------------------------------------------------------------
_WORDS = ["great", "don't", "it's", "bad", "value", "na\u00efve", "caf\u00e9", "\u0130stanbul",
          "\u4e2d\u6587", "\U0001f600", "\U0001f44d\U0001f3fd", "quote\"inside", "back\\slash",
          "tab\there", "line\nbreak", "\u2028", "slash/", "\x7f", "K\u212a", "end\\"]


def _sentence(rng, lo=0, hi=12) -> str:
    return " ".join(rng.choice(_WORDS) for _ in range(rng.randint(lo, hi)))


def _review(rng, users, items) -> dict:
    r = {"user_id": rng.choice(users), "parent_asin": rng.choice(items),
         "rating": rng.choice([1.0, 2.0, 3.0, 4.0, 5.0, 4.5, 3.75, 5, 1, 0.5, 4.35]),
         "helpful_vote": rng.choice([0, 0, 1, 7, 123456, -2]),
         "verified_purchase": rng.random() < 0.7,
         "timestamp": rng.choice([1588687728923, 1609459200000, 1234567, -5, 1700000000123]),
         "title": _sentence(rng, 0, 4), "text": _sentence(rng),
         "asin": "B0" + str(rng.randint(0, 99)),
         "images": [{"text": "nested", "rating": 9, "user_id": "nested", "parent_asin": "n",
                     "url": "https://x/y.jpg", "sizes": [1, [2, {"title": "deep"}]]}
                    for _ in range(rng.randint(0, 2))]}
    roll = rng.random()
    if roll < 0.04:
        r["rating"] = None
    elif roll < 0.08:
        r["user_id"] = ""
    elif roll < 0.12:
        del r["parent_asin"]
    elif roll < 0.16:
        r["title"] = None
    elif roll < 0.20:
        del r["helpful_vote"], r["timestamp"], r["verified_purchase"], r["text"]
    elif roll < 0.24:
        r["timestamp"] = r["helpful_vote"] = r["verified_purchase"] = None
    return r


def _dumps(rng, r: dict) -> bytes:
    ks = list(r)
    rng.shuffle(ks)
    s = json.dumps({k: r[k] for k in ks}, ensure_ascii=rng.random() < 0.5,
                   separators=rng.choice([(",", ":"), (", ", ": ")]))
    return s.encode("utf-8", "surrogatepass")


def plain_corpus(n: int = 120, seed: int = 7) -> bytes:
    """``json.dumps`` of random well-formed reviews: both ``ensure_ascii``
    settings, both separator styles, shuffled keys, nested objects that hold
    the keys read, non-ASCII text and emoji, few users and items (repeats far
    apart), skipped records. The device's rule flags none of its lines."""
    rng = random.Random(seed)
    users = ["AE%05d" % rng.randint(0, 99999) for _ in range(17)] + ["\u00fcser", "u\U0001f600"]
    items = ["B%09d" % rng.randint(0, 10**9) for _ in range(11)] + ["\u54c1"]
    return b"".join(_dumps(rng, _review(rng, users, items)) + b"\n" for _ in range(n))


def many_ids_corpus(n: int = 300) -> bytes:
    """n records of n distinct users and n distinct items, some met again: more
    ids than an 8-bit hash has values, so under that mask two must share one."""
    lines = [b'{"user_id":"U%03d","parent_asin":"P%d","rating":%d}' % (k, 7 * k, k % 5 + 1)
             for k in range(n)]
    lines += [b'{"user_id":"U%03d","parent_asin":"P%d","rating":3}' % (k, 7 * (n - 1 - k))
              for k in range(0, n, 9)]
    return b"\n".join(lines) + b"\n"


_OK = '"user_id":"u1","parent_asin":"i1","rating":5'
# Lines the host reader accepts (it may skip them); the device flags some.
ODD_LINES = [
    b'{"user\\u005fid":"esc","user_id":"u0","parent_asin":"i1","rating":5}',      # key with a backslash
    b'{"user_id":"u1","parent_asin":"i1","rating":NaN}',
    b'{"user_id":"u1","parent_asin":"i1","rating":1e0}',
    b'{"user_id":"u1","parent_asin":"i1","rating":5.0E+0}',
    b'{"user_id":"u1","parent_asin":"i1","rating":4.35}',
    b'{"user_id":"u1","parent_asin":"i2","rating":5}',
    b'{"user_id":"u2","parent_asin":"i1","rating":-0}',
    b'{"user_id":"u2","parent_asin":"i1","rating":-0.0}',
    b'{"user_id":"u2","parent_asin":"i1","rating":-1.5}',
    b'{"user_id":"u2","parent_asin":"i1","rating":4.1234567890123456}',            # 17 digits
    b'{"user_id":"u2","parent_asin":"i1","rating":123456789012345}',               # 15 digits
    b'{"user_id":"u2","parent_asin":"i1","rating":0.000000000000001}',
    b'{"user_id":"u2","parent_asin":"i1","rating":"4.5"}',
    b'{"user_id":"u2","parent_asin":"i1","rating":true}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":null}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":3.0}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":"7"}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":2147483647}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":-2147483648}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"helpful_vote":[1]}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"timestamp":999999999999999999}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"timestamp":1000000000000000000}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"timestamp":-12,"verified_purchase":1}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"timestamp":1.5e3,"verified_purchase":"yes"}',
    b'{"user_id":"u3","parent_asin":"i3","rating":3,"timestamp":null,"verified_purchase":null}',
    b'{"user_id":"u4","parent_asin":"i4","rating":2,"text":"bad \xff utf8 \xc3"}',  # malformed UTF-8
    b'{"user_id":"u4\xed\xa0\x80","parent_asin":"i4","rating":2}',                 # a raw surrogate
    b'{"user_id":"u4","parent_asin":"i4","rating":2,"rating":4,"text":"a","text":"b"}',   # duplicates
    b'{"user_id":"u4","parent_asin":"i4","rating":2,"user_id":"u1"}',
    b'\xc2\xa0',                                                                     # U+00A0 alone
    b'\x0c',
    b'',
    b'   \t ',
    b'{"user_id":"u5","parent_asin":"i5","rating":1}\r',                            # \r\n
    b'{"user_id":"lone\\ud83d","parent_asin":"i5","rating":1,"text":"x\\udc00y"}',
    b'{"user_id":"pair\\ud83d\\ude00","parent_asin":"i5","rating":1,"text":"\\uD83D\\uDE00!"}',
    b'{"user_id":"u5","parent_asin":"i5","rating":1,"text":"\\ud83d\\u0041\\ud83d\\ud83d\\ude00"}',
    b'{"user_id":"u5","parent_asin":"i5","rating":1,"text":"\\u0000\\u00e9\\u20ac\\/\\b\\f\\n\\r\\t"}',
    b'{"user_id":"u5","parent_asin":"i5","rating":1,"text":"q\\\\\\" w\\\\\\\\","title":"\\\\"}',
    b'  { "user_id" : "u6" ,\t"parent_asin"\t:\t"i6" , "rating" : 4.0 }  \t',
    b'{"meta":{"rating":1,"user_id":"x","text":"no"},"user_id":"u6","parent_asin":"i6","rating":3}',
    b'{"a":[{"user_id":"x"},["rating",{"rating":2}]],"user_id":"u6","parent_asin":"i6","rating":3}',
    b'{"note":"a } ] : { \\" [","user_id":"u6","parent_asin":"i6","rating":3}',
    b'{}',
    b'{"user_id":null,"parent_asin":"i6","rating":3}',
    b'{"user_id":"u6","parent_asin":"","rating":3}',
    b'{"user_id":"u6","parent_asin":"i6","rating":null,"title":5}',                 # skipped before the join
    b'{"user_id":"u1","parent_asin":"i1","rating":5,"title":null,"text":null}',
    b'{"user_id":"u7","parent_asin":"i7","rating":5,"title":"","text":""}',
]
ODD_LAST = b'{"user_id":"u8","parent_asin":"i1","rating":2.5,"text":"no newline at the end"}'

# Lines on which the host reader raises; each is tested in a file of its own.
ODD_RAISING = [
    b'{"user_id":"u1","parent_asin":"i1","rating":5,"text":"\\x41"}',     # invalid escape
    b'{"user_id":"u1","parent_asin":"i1","rating":5,"text":"\\u12G4"}',
    b'[1, 2]',                                                             # no '{'
    b'\xef\xbb\xbf{' + _OK.encode() + b'}',                                # a BOM
    b'{' + _OK.encode() + b',"a":[1}',                                     # unbalanced
    b'{' + _OK.encode() + b',"a":1]',
    b'{' + _OK.encode() + b',"text":"open}',                               # unterminated string
    b'{' + _OK.encode() + b'} x',                                          # bytes after the close
    b'{' + _OK.encode() + b'}{' + _OK.encode() + b'}',
    b'{' + _OK.encode() + b',"text":"a\tb"}',                              # a raw tab in a string
    b'{' + _OK.encode() + b',"helpful_vote":2147483648}',                  # outside int32
    b'{' + _OK.encode() + b',"title":5}',
    b'{"user_id":"u1","parent_asin":"i1","rating":"abc"}',
    b'{"user_id":"u1","parent_asin":"i1","rating":[5]}',
    b'{"user_id":["u1"],"parent_asin":"i1","rating":5}',
    b'{' + _OK.encode() + b',"verified_purchase":trueX}',                  # bytes stuck to a value read
    b'{' + _OK.encode() + b',"timestamp":null5}',
    b'{"user_id":"a"junk,"parent_asin":"i1","rating":5}',
    b'{' + _OK.encode() + b',"text":"t""u"}',
]


def odd_corpus() -> bytes:
    """One line per form the device flags (and the host accepts), duplicate
    keys, ``\\r\\n``, a lone ``\\r`` between two objects, blank lines, U+00A0,
    surrogates, the number forms, and a last line without a newline."""
    lone_cr = b'{"user_id":"u9","parent_asin":"i9","rating":1}\r{"user_id":"u9","parent_asin":"i1","rating":2}'
    return b"\n".join(ODD_LINES + [lone_cr]) + b"\n\n" + ODD_LAST


_VALUES = [None, True, False, 0, 1, -1, 5, 2**31 - 1, 2**31, -2**31 - 1, 10**17, 10**18, 10**30,
           0.0, 4.5, 3.25, 1e-7, 1e22, 123456.789, "", "x", "4", "4.5", " 7 ", "nan", "u\u00e9",
           "\U0001f600", "a\"b\\c", "\ud83d", [], [1, "a"], {}, {"rating": 1, "text": "t"}]
_LITERALS = ["1e0", "-0", "-0.0", "4.350", "0.5", "-1.25", "5.0E+0", "NaN", "Infinity", "1E2",
             "123456789012345678", "1234567890123456789", "0.1234567890123456", "12345.6789"]


def random_lines(n: int = 2000, seed: int = 3) -> list:
    """Valid JSON lines with any value type or number form under any key."""
    rng = random.Random(seed)
    keys = ["user_id", "parent_asin", "rating", "helpful_vote", "verified_purchase", "timestamp",
            "title", "text", "other"]
    good = {"user_id": ["a", "b", "c\u00e9"], "parent_asin": ["p", "q"], "rating": [1, 4.5, 3.0],
            "helpful_vote": [0, 3, None], "verified_purchase": [True, False, None],
            "timestamp": [1588687728923, -4, None], "other": [1, "x", None]}
    out = []
    for _ in range(n):
        r, marks = {}, {}
        for k in keys:
            roll = rng.random()
            if roll < 0.08:
                continue
            if roll < 0.88:
                r[k] = _sentence(rng, 0, 5) if k in ("title", "text") else rng.choice(good[k])
            elif roll < 0.94:
                marks[k] = rng.choice(_LITERALS)
                r[k] = "@@%s@@" % k
            else:
                r[k] = rng.choice(_VALUES)
        line = _dumps(rng, r).decode("utf-8", "surrogatepass")
        for k, lit in marks.items():
            line = line.replace('"@@%s@@"' % k, lit)
        if rng.random() < 0.1:
            line = '{"user_id": "dup", ' + line.lstrip()[1:]
        out.append(line.encode("utf-8", "surrogatepass"))
    return out
