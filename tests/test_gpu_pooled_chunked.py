"""GPU: the regrouped pooled count, bbgr.text.pooled_token_counts(..,
chunk_bytes=c), and build_credibility_graph(.., feature_set="v2",
text_chunk_bytes=c): the same bits as the one-chunk call and the host
restatement tests/features_v2_ref.py on the corpus of
tests/test_gpu_features_v2.py, at chunk sizes below and above the hub user's
text, and on a text of more than 2^32 bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import features_v2_ref as V  # noqa: E402
import jsonl_ref as R  # noqa: E402

DEV = "cuda"
U, I = V.U, V.I
TENSORS = ("src", "dst", "edge_attr", "user_x", "user_y", "item_x", "total_reviews",
           "helpful_reviews", "user_extra")


def _np(t):
    return t.cpu().numpy()


def _columns(ns):
    from bbgr.features import ReviewColumns
    from bbgr.text import ReviewText
    return ReviewColumns(user=ns.user, item=ns.item, rating=ns.rating,
                         helpful_vote=ns.helpful_vote, verified=ns.verified,
                         timestamp=ns.timestamp, ts_valid=ns.ts_valid,
                         text=ReviewText(ns.text.data, ns.text.offsets))


def _build(cols, n_users=U, n_items=I, **kw):
    from bbgr.features import build_credibility_graph
    return build_credibility_graph(cols, n_users, n_items, device=DEV, **kw)


def _same_graph(a, b):
    assert type(a) is type(b)
    for key in TENSORS:
        x, y = getattr(a, key), getattr(b, key)
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert _np(x).tobytes() == _np(y).tobytes(), key       # bit for bit, the NaN rows too
    assert a.stats == b.stats


@pytest.fixture(scope="module")
def case():
    """The corpus, the restatement, the one-chunk count and the default v2 build, once."""
    from bbgr.text import ReviewText, pooled_token_counts
    ns = V.corpus_columns(V.gpu_corpus())
    ref = V.features_v2_ref(ns, U, I)
    text = ReviewText(ns.text.data, ns.text.offsets)
    cols = _columns(ns)
    return ns, text, ref, pooled_token_counts(text, ns.user, U, DEV), cols, \
        _build(cols, feature_set="v2")


def _planned(ns, chunk_bytes):
    from bbgr.text import plan_group_ranges
    sizes = np.bincount(ns.user, weights=np.diff(ns.text.offsets), minlength=U).astype(np.int64)
    return sizes, plan_group_ranges(np.concatenate([[0], np.cumsum(sizes)]), chunk_bytes)


@pytest.mark.parametrize("chunk_bytes", [1, 4096, 65536, 1 << 20, 1 << 30])
def test_chunked_equals_one_chunk_and_the_restatement(case, chunk_bytes):
    from bbgr.text import pooled_token_counts
    ns, text, ref, (tok1, uniq1, info1), _, _ = case
    tok, uniq, info = pooled_token_counts(text, ns.user, U, DEV, chunk_bytes=chunk_bytes)
    assert tok.dtype == torch.int64 and uniq.dtype == torch.int32 and tok.is_cuda
    np.testing.assert_array_equal(_np(tok), ref["pooled_tokens"])
    np.testing.assert_array_equal(_np(uniq), ref["pooled_unique"])
    assert torch.equal(tok, tok1) and torch.equal(uniq, uniq1)
    sizes, plan = _planned(ns, chunk_bytes)
    assert info.pop("chunks") == len(plan)
    assert info == info1 and list(info) == list(info1)
    if chunk_bytes < int(sizes[0]):
        assert (0, 1) in plan                                  # the hub user runs alone
    else:
        assert plan[0][1] > 1


def test_a_narrow_hash_still_counts_exactly(case):
    from bbgr.text import pooled_token_counts
    ns, text, ref, (tok1, uniq1, info1), _, _ = case
    _, _, one8 = pooled_token_counts(text, ns.user, U, DEV, _hash_mask=0xFF)
    tok8, uniq8, info8 = pooled_token_counts(text, ns.user, U, DEV, _hash_mask=0xFF,
                                             chunk_bytes=4096)
    assert torch.equal(tok8, tok1) and torch.equal(uniq8, uniq1)
    assert info8["rechecked"] == one8["rechecked"] > info1["rechecked"]
    assert info8["kelvin_records"] == one8["kelvin_records"]


def test_groups_on_the_device_and_out_views(case):
    from bbgr.text import pooled_token_counts
    ns, text, _, (tok1, uniq1, _), _, _ = case
    big_t = torch.full((U + 64,), -7, dtype=torch.int64, device=DEV)
    big_u = torch.full((U + 64,), -7, dtype=torch.int32, device=DEV)
    tok_v, uniq_v, _ = pooled_token_counts(text, torch.as_tensor(ns.user).to(DEV), U, DEV,
                                           out=(big_t[:U], big_u[:U]), chunk_bytes=65536)
    assert torch.equal(tok_v, tok1) and torch.equal(uniq_v, uniq1)
    assert tok_v.data_ptr() == big_t.data_ptr()
    assert bool((big_t[U:] == -7).all()) and bool((big_u[U:] == -7).all())
    with pytest.raises(ValueError, match="group id out of range"):
        pooled_token_counts(text, np.where(ns.user == 3, U, ns.user), U, DEV, chunk_bytes=4096)
    with pytest.raises(ValueError, match="chunk_bytes"):
        pooled_token_counts(text, ns.user, U, DEV, chunk_bytes=0)


def test_the_text_on_the_device_and_a_group_csr(case):
    """A device-resident text is used where it is, and a caller's CSR of the
    records by group (bbgr_csr_build with the record id as the column)."""
    from bbgr.features import _group
    from bbgr.text import pooled_token_counts, resident
    ns, text, _, (tok1, uniq1, info1), _, _ = case
    there = resident(text, DEV)
    assert there.data.is_cuda and resident(there, DEV).data.data_ptr() == there.data.data_ptr()
    user = torch.as_tensor(ns.user).to(DEV)
    csr = _group(user, torch.zeros_like(user), U)
    tok, uniq, info = pooled_token_counts(there, user, U, DEV, chunk_bytes=65536, group_csr=csr)
    assert torch.equal(tok, tok1) and torch.equal(uniq, uniq1)
    assert {k: v for k, v in info.items() if k != "chunks"} == info1


def test_a_host_text_inside_a_longer_array(case):
    """Bytes before the first record and behind the last are no text: words
    there are not counted, as a host array and as a device tensor."""
    from bbgr.text import ReviewText, pooled_token_counts
    ns, _, _, (tok1, uniq1, info1), _, _ = case
    junk = np.frombuffer(b"never counted words ", np.uint8)
    data = np.concatenate([np.tile(junk, 5), ns.text.data, np.tile(junk, 3)])
    off = np.asarray(ns.text.offsets) + 5 * junk.size
    for d in (data, torch.from_numpy(data).to(DEV)):
        tok, uniq, info = pooled_token_counts(ReviewText(d, off), ns.user, U, DEV,
                                              chunk_bytes=65536)
        assert torch.equal(tok, tok1) and torch.equal(uniq, uniq1)
        assert info["rechecked"] == info1["rechecked"] and info["tokens"] == info1["tokens"]


def test_text_of_more_than_4_gib(case):
    """The corpus's records at offsets spread over 2^32 + 2^24 zero bytes made
    on the device: record 2r is corpus record r, record 2r + 1 the zeros up to
    the next. The issue puts all the zeros into one filler group; a group of
    2^31 - 1 bytes or more is a ValueError by the same issue, so the fillers
    take three groups behind the users, each below that, by thirds of the
    records. Every filler group counts 0 tokens, every user as the
    restatement; the one-chunk call refuses the text by its size."""
    from bbgr.text import BYTES_MAX, ReviewText, pooled_token_counts
    ns, _, ref, _, _, _ = case
    old = np.asarray(ns.text.offsets)
    n = old.size - 1
    lens = np.diff(old)
    N = 2**32 + 2**24
    gap = (N - int(old[-1])) // n
    off = np.zeros(2 * n + 1, np.int64)
    off[1::2] = lens
    off[2::2] = gap
    off[-1] += N - int(old[-1]) - gap * n                      # the last filler ends the text
    off = np.concatenate([[0], np.cumsum(off[1:])])
    assert off[-1] == N and N > 2**32
    group = np.empty(2 * n, np.int32)
    group[0::2] = ns.user
    group[1::2] = U + np.arange(n) * 3 // n                    # fillers: groups U, U + 1, U + 2
    filler = np.bincount(group[1::2] - U, weights=np.diff(off)[1::2])
    assert filler.size == 3 and filler.max() < BYTES_MAX and filler.sum() > 2**32
    # the bytes: zeros, then every corpus byte moved to its record's new start
    data = torch.zeros(N, dtype=torch.uint8, device=DEV)
    shift = torch.from_numpy(off[0:-1:2] - old[:-1]).to(DEV)
    at = torch.repeat_interleave(shift, torch.from_numpy(lens).to(DEV)) + \
        torch.arange(int(old[-1]), device=DEV)
    data[at] = torch.from_numpy(np.asarray(ns.text.data)).to(DEV)
    text = ReviewText(data, off)
    tok, uniq, info = pooled_token_counts(text, group, U + 3, DEV, chunk_bytes=1 << 20)
    np.testing.assert_array_equal(_np(tok[:U]), ref["pooled_tokens"])
    np.testing.assert_array_equal(_np(uniq[:U]), ref["pooled_unique"])
    assert _np(tok[U:]).tolist() == [0, 0, 0] and _np(uniq[U:]).tolist() == [0, 0, 0]
    assert info["rechecked"] == len(V.KELVIN_RECORDS)
    assert info["kelvin_records"] == sum(V.KELVIN_RECORDS.values())
    assert info["tokens"] == int(ref["pooled_tokens"].sum()) and info["chunks"] >= 6
    with pytest.raises(ValueError, match=r"2\^31 - 1 bytes"):
        pooled_token_counts(text, group, U + 3, DEV)
    with pytest.raises(ValueError, match=r"group 300 has \d+ bytes"):
        pooled_token_counts(text, np.minimum(group, U), U + 1, DEV, chunk_bytes=1 << 20)


@pytest.mark.parametrize("chunk_bytes", [4096, 1 << 20])
def test_the_v2_build_is_the_same(case, chunk_bytes):
    _, _, _, _, cols, out = case
    again = _build(cols, feature_set="v2", text_chunk_bytes=chunk_bytes)
    _same_graph(again, out)


def test_two_chunked_builds_are_bitwise_identical(case):
    _, _, _, _, cols, _ = case
    _same_graph(_build(cols, feature_set="v2", text_chunk_bytes=65536),
                _build(cols, feature_set="v2", text_chunk_bytes=65536))


def test_main_ignores_the_argument(case):
    from bbgr.features import CredibilityGraph
    _, _, _, _, cols, _ = case
    a, b = _build(cols), _build(cols, feature_set="main", text_chunk_bytes=4096)
    assert type(a) is CredibilityGraph and type(b) is CredibilityGraph
    for key in TENSORS[:-1]:
        assert _np(getattr(a, key)).tobytes() == _np(getattr(b, key)).tobytes(), key
    assert a.stats == b.stats


def test_a_text_chunk_below_one_is_refused(case):
    _, _, _, _, cols, _ = case
    with pytest.raises(ValueError, match="text_chunk_bytes"):
        _build(cols, feature_set="v2", text_chunk_bytes=0)


def test_jsonl_to_v2_chunked():
    """A dump parsed in several chunks, its device-resident text regrouped in
    chunks of 4096 bytes: the default v2 build of the same parse."""
    from bbgr import jsonl
    data = R.plain_corpus()
    parsed = jsonl.read_reviews(data, chunk_bytes=max(len(data) // 5, 2000))
    assert parsed.info["chunks"] > 1 and parsed.cols.text.data.is_cuda
    n_users, n_items = len(parsed.user_ids), len(parsed.item_ids)
    want = _build(parsed.cols, n_users, n_items, feature_set="v2")
    got = _build(parsed.cols, n_users, n_items, feature_set="v2", text_chunk_bytes=4096)
    _same_graph(got, want)
    assert torch.isfinite(got.user_x).all() and torch.isfinite(got.user_extra).all()
