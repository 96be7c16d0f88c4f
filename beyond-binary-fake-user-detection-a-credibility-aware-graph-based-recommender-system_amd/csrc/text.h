// What the kernels that read review text share (text.hip, features_v2.hip):
// the letter rule, a record's clamped byte range, the cursor that reads a
// token's normalised bytes forward from its start, the token stream of
// bbgr_text_unique's EMIT stage and where that stage leaves it in the
// workspace.
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

// The carve of bbgr_text_unique's workspace up to the sort's own temporary
// storage: token offsets [n + 1], then per token its record, its start, the
// hash and the token index before (k1, v1) and after (k2, v2) the sort.
struct TextWorkspace {
  size_t off_rec, off_pos, off_k1, off_k2, off_v1, off_v2, off_tmp;
};

inline TextWorkspace text_workspace(long n, size_t nt) {
  TextWorkspace w;
  w.off_rec = align_up(sizeof(int) * (size_t)(n + 1));
  w.off_pos = w.off_rec + align_up(sizeof(int) * nt);
  w.off_k1 = w.off_pos + align_up(sizeof(uint32_t) * nt);
  w.off_k2 = w.off_k1 + align_up(sizeof(unsigned long long) * nt);
  w.off_v1 = w.off_k2 + align_up(sizeof(unsigned long long) * nt);
  w.off_v2 = w.off_v1 + align_up(sizeof(uint32_t) * nt);
  w.off_tmp = w.off_v2 + align_up(sizeof(uint32_t) * nt);
  return w;
}

}  // namespace bbgr
