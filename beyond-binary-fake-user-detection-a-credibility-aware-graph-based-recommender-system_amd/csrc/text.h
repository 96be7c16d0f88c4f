// What the kernels that read review text share (text.hip, features_v2.hip):
// the letter rule, a record's clamped byte range, the cursor that reads a
// token's normalised bytes forward from its start, the token stream of
// bbgr_text_unique's EMIT stage and where that stage leaves it in the
// workspace, and the rule of the distinct count (per record there, per group
// here): the comparison of two tokens, the count per run of equal keys in a
// wave, the clamped row bounds of the segmented sorts, the flag total.
#pragma once

#include "common.h"

namespace bbgr {

__device__ __forceinline__ bool text_ascii_letter(unsigned b) {
  const unsigned lo = b | 0x20u;   // A-Z onto a-z; no other byte lands inside a-z
  return lo >= 'a' && lo <= 'z';
}

// The record's byte range, clamped into [first, last): no offset, however
// wrong, sends a read outside the text.
__device__ __forceinline__ void text_range(const long long *offsets, long r, long first, long last,
                                           long &beg, long &end) {
  beg = (long)offsets[r];
  end = (long)offsets[r + 1];
  beg = beg < first ? first : beg;
  end = end > last ? last : end;
}

// A token read forward from its first byte: next() gives its normalised bytes
// (lower-case letters, the apostrophe between its two parts) and -1 at its end.
struct TokenCursor {
  const uint8_t *d;
  long q, end;
  bool second;
  __device__ __forceinline__ int letter(long at) const {
    const unsigned b = d[at];
    if (text_ascii_letter(b)) return (int)(b | 0x20u);
    if (b == 0xC4u && at + 1 < end && d[at + 1] == 0xB0u) return 'i';
    return 0;
  }
  __device__ __forceinline__ int next() {
    if (q >= end) return -1;
    const int c = letter(q);
    if (c) {
      ++q;
      return c;
    }
    if (!second && d[q] == 0x27u && q + 1 < end && letter(q + 1)) {
      second = true;
      ++q;
      return 0x27;
    }
    return -1;
  }
};

struct TextTokens {
  long n;
  long total;   // the caller's count; the kernels stop at the scan's own, tok_off[n], if smaller
  const uint8_t *data;
  const long long *offsets;
  long first, last;
  const uint32_t *tok_pos;
  const int *tok_rec;
  const int *tok_off;
  unsigned long long hash_mask;
};

__device__ __forceinline__ long text_live_tokens(const TextTokens &T) {
  const long scanned = T.tok_off[T.n];
  return scanned < T.total ? scanned : T.total;
}

// A slot or a record out of range (n_tokens changed between the two calls)
// reads as an empty token.
__device__ __forceinline__ TokenCursor text_cursor(const TextTokens &T, long tok) {
  if (tok < 0 || tok >= T.total) return TokenCursor{T.data, 0, 0, false};
  const int rec = T.tok_rec[tok];
  if (rec < 0 || rec >= T.n) return TokenCursor{T.data, 0, 0, false};
  long beg, end;
  text_range(T.offsets, rec, T.first, T.last, beg, end);
  long q = T.first + (long)T.tok_pos[tok];
  return TokenCursor{T.data, q < end ? q : end, end, false};
}

// Whether the normalised bytes of tokens a and b differ, read side by side to
// their ends.
__device__ __forceinline__ bool text_tokens_differ(const TextTokens &T, long a, long b) {
  TokenCursor ca = text_cursor(T, a), cb = text_cursor(T, b);
  for (;;) {
    const int x = ca.next(), y = cb.next();
    if (x != y) return true;
    if (x < 0) return false;
  }
}

// The distinct count of one lane per sorted slot, called by the whole wave:
// key is the slot's record or group (live: it has one; every other lane holds
// a key no live lane has), opens whether the slot begins a run of equal
// tokens. The lanes of a wave that share a key add their opening slots to
// count[key] with one integer atomic, issued by the first of them.
__device__ __forceinline__ void text_count_opens(int key, bool live, bool opens, int *count) {
  const int lane = threadIdx.x & 63;
  const int left = __shfl_up(key, 1);
  const unsigned long long heads = __ballot(lane == 0 || key != left), open_m = __ballot(opens);
  if (live && (heads >> lane & 1ull)) {
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = after ? __ffsll((long long)after) : 64 - lane;   // lanes of this key here
    const unsigned long long mine = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
    const int cnt = __popcll(open_m & mine);
    if (cnt) atomicAdd(count + key, cnt);
  }
}

// Row bounds of a segmented sort from an indptr (a CSR's, or the token
// offsets): row r is [begin(r), end(r)), both clamped into [0, n] and end(r)
// >= begin(r), so no indptr, however wrong (a workspace no scan has filled),
// sends the sort outside its keys.
struct RowBound {
  const int *indptr;
  int n;
  bool end;
  __host__ __device__ __forceinline__ int clamp(int v) const { return v < 0 ? 0 : (v < n ? v : n); }
  __host__ __device__ __forceinline__ int operator()(int r) const {
    const int b = clamp(indptr[r]);
    if (!end) return b;
    const int e = clamp(indptr[r + 1]);
    return e < b ? b : e;
  }
};

// The carve of bbgr_text_unique's workspace up to the sort's own temporary
// storage: token offsets [n + 1], then per token its record, its start, the
// hash and the token index before (k1, v1) and after (k2, v2) the sort.
struct TextWorkspace {
  size_t off_tok, off_rec, off_pos, off_k1, off_k2, off_v1, off_v2, off_tmp;
};

inline TextWorkspace text_workspace(long n, size_t nt) {
  TextWorkspace w;
  Carver C;
  w.off_tok = C.take_n<int>((size_t)(n + 1));
  w.off_rec = C.take_n<int>(nt);
  w.off_pos = C.take_n<uint32_t>(nt);
  w.off_k1 = C.take_n<unsigned long long>(nt);
  w.off_k2 = C.take_n<unsigned long long>(nt);
  w.off_v1 = C.take_n<uint32_t>(nt);
  w.off_v2 = C.take_n<uint32_t>(nt);
  w.off_tmp = C.used;
  return w;
}

// The token stream of T tokens that the EMIT stage leaves (or will leave) in
// `workspace`.
inline TextTokens text_tokens(const bbgr_text_args *a, void *workspace, const TextWorkspace &W,
                              int T) {
  TextTokens K;
  K.n = (long)a->n;
  K.total = T;
  K.data = a->data;
  K.offsets = reinterpret_cast<const long long *>(a->offsets);
  K.first = (long)a->first;
  K.last = (long)a->last;
  K.tok_pos = ws_at<const uint32_t>(workspace, W.off_pos);
  K.tok_rec = ws_at<const int>(workspace, W.off_rec);
  K.tok_off = ws_at<const int>(workspace, W.off_tok);
  K.hash_mask = a->hash_mask ? a->hash_mask : ~0ull;
  return K;
}

// text.hip: the checks of bbgr_text_args every entry point that takes one
// shares, and totals[1] += the number of non-zero flag[0 .. n) (one launch of
// text_recheck_total_kernel).
int text_check(const char *fn, const bbgr_text_args *a);
int text_flag_total(long n, const uint8_t *flag, int64_t *totals, hipStream_t st);

}  // namespace bbgr
