// The review dump (one JSON object per line) -> per-record columns, id bytes
// and text bytes, and the numbering of id strings by first appearance
// (features.review_columns_from_jsonl, restated over bytes).
//
// Lines. '\n' and '\r' both terminate a line; a last line without a terminator
// counts. jsonl_tile_kernel: one wave per tile of 4096 bytes in 64-byte steps,
// a ballot of the terminators per step; COUNT leaves the tile's count, SCATTER
// (after an exclusive scan of the counts) writes each terminator's position at
// its rank: line_end[l], line l = data[line_end[l - 1] + 1, line_end[l]).
//
// Structure. jsonl_scan_kernel: one wave per line, 64 bytes a step, a byte a
// lane. Ballots of '\\' and '"' give, with the carried escape parity, the
// unescaped quotes Q; a prefix xor of Q (and the carried in-string bit) the
// string mask; ballots of the brackets outside strings and a popcount below
// the lane the depth before every byte. A ':' outside strings at depth 1 ends
// a top-level key: its lane walks back over the key (a key with a backslash
// flags the line), compares it with the eight keys read, and skips forward to
// the value; per key the last such lane of the step wins (the last occurrence
// of a key wins, as in dict). Deeper keys are never looked at. The line is
// flagged for: a first byte that is not '{', a byte below 0x20 other than a tab
// outside strings, a backslash outside strings, an unterminated string,
// unbalanced brackets, a top-level close that is not '}', bytes after it.
//
// Values. Lanes 0 .. 7 then read one value each, serially from its first byte
// (jl_string, jl_number): the forms the header lists are vouched for, every
// other flags the line. A flagged line is parsed by the caller on the host,
// who hands its values and bytes back through `side` (status 4).
//
// bbgr_jsonl_offsets: exclusive scans of the kept flags and the three sizes.
// jsonl_write_kernel: one wave per kept line; lane 0 the numeric columns,
// lanes 0 .. 3 the unescaped user id, item id, title and text (jl_string
// again, now with an output), or for status 4 a copy out of `side`.
//
// bbgr_ids_number: FNV-1a + finaliser per id string, a stable radix sort of
// (hash, record), per sorted slot a comparison of the string with its left
// neighbour's where the hashes are equal (an unequal pair counts in
// totals[1]: the caller then numbers on the host), run heads, a scan of the
// heads in record order: the id of every run, of every record, and the record
// of every id's first appearance, from which bbgr_ids_table copies the table.
//
// Integer and exact-double work only (a rating is (double)digits / 10^k, one
// correctly rounded division, then one cast to float); integer atomics add
// order-free counts: two calls give the same bits. Every offset, position and
// index read from a workspace or a caller's buffer is clamped or checked
// before it addresses anything.
#include "cub_temp.h"


namespace bbgr {

constexpr int JL_WAVES = 4;            // lines (tiles) in flight per workgroup of 256 threads
constexpr long JL_MAX_BLOCKS = 16384;
constexpr int JL_TILE = 4096;          // bytes of a line-finding tile
constexpr long JL_N_MAX = 2147483647LL;

enum { JL_BLANK = 0, JL_SKIPPED = 1, JL_KEPT = 2, JL_FLAGGED = 3, JL_HOST = 4 };

typedef bbgr_jsonl_args JsonlParams;

__device__ __forceinline__ bool jl_term(unsigned b) { return b == '\n' || b == '\r'; }
__device__ __forceinline__ bool jl_blank(unsigned b) { return b == ' ' || b == '\t'; }
__device__ __forceinline__ bool jl_digit(unsigned b) { return b >= '0' && b <= '9'; }
// A value ends at a blank, ',' or '}' inside the line.
__device__ __forceinline__ bool jl_ends(const uint8_t *d, long i, long end) {
  return i < end && (jl_blank(d[i]) || d[i] == ',' || d[i] == '}');
}

__device__ __forceinline__ long jl_clamp(long v, long lo, long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// ---------------------------------------------------------------------------
// lines
// ---------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(64 * JL_WAVES) void jsonl_tile_kernel(long n_bytes,
                                                                   const uint8_t *data,
                                                                   long n_tiles, int *tile_count,
                                                                   const int *tile_off,
                                                                   long n_lines, int *line_end,
                                                                   long long *totals) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * JL_WAVES + (threadIdx.x >> 6);
  const long n_waves = (long)gridDim.x * JL_WAVES;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long t = wave; t < n_tiles; t += n_waves) {
    const long beg = t * JL_TILE;
    const long end = beg + JL_TILE < n_bytes ? beg + JL_TILE : n_bytes;
    long rank = SCATTER ? (long)tile_off[t] : 0;
    for (long base = beg; base < end; base += 64) {
      const long p = base + lane;
      const bool term = p < end && jl_term(data[p]);
      const unsigned long long T = __ballot(term);
      if (SCATTER && term) {
        const long at = rank + __popcll(T & below);
        if (at >= 0 && at < n_lines) line_end[at] = (int)p;
      }
      rank += __popcll(T);
      if (p == n_bytes - 1 && !term) {   // the last line has no terminator
        if (SCATTER) {
          const long at = rank;          // every terminator lies before it
          if (at >= 0 && at < n_lines) line_end[at] = (int)n_bytes;
        } else if (totals) {
          atomicAdd(reinterpret_cast<unsigned long long *>(totals), 1ull);
        }
      }
    }
    if (!SCATTER && lane == 0) {
      if (tile_count) tile_count[t] = (int)rank;
      if (rank && totals) atomicAdd(reinterpret_cast<unsigned long long *>(totals), (unsigned long long)rank);
    }
  }
}

// ---------------------------------------------------------------------------
// values
// ---------------------------------------------------------------------------
__device__ __forceinline__ int jl_hex4(const uint8_t *d, long i) {
  int v = 0;
  for (int k = 0; k < 4; ++k) {
    const unsigned c = d[i + k];
    int h;
    if (c >= '0' && c <= '9') h = (int)c - '0';
    else if ((c | 0x20u) >= 'a' && (c | 0x20u) <= 'f') h = (int)(c | 0x20u) - 'a' + 10;
    else return -1;
    v = v << 4 | h;
  }
  return v;
}

// The JSON string whose opening quote is d[q], inside [q, end): its size after
// unescaping, or -1 when it is not vouched for (a byte below 0x20, an escape
// outside \" \\ \/ \b \f \n \r \t \uXXXX, UTF-8 that Python's strict decoder
// refuses, no closing quote before `end`). A high + low \u surrogate pair is
// one 4-byte code point, a lone surrogate its 3 surrogatepass bytes. With
// `out` the bytes are written, those below `cap`; `after` receives the
// position behind the closing quote.
__device__ long jl_string(const uint8_t *d, long q, long end, uint8_t *out, long cap,
                          long *after = nullptr) {
  long i = q + 1, o = 0;
  auto put = [&](unsigned c) {
    if (out && o < cap) out[o] = (uint8_t)c;
    ++o;
  };
  for (;;) {
    if (i >= end) return -1;
    const unsigned c = d[i];
    if (c == '"') {
      if (after) *after = i + 1;
      return o;
    }
    if (c < 0x20u) return -1;
    if (c == '\\') {
      if (i + 1 >= end) return -1;
      const unsigned e = d[i + 1];
      i += 2;
      if (e == 'u') {
        if (i + 4 > end) return -1;
        int cp = jl_hex4(d, i);
        if (cp < 0) return -1;
        i += 4;
        if (cp >= 0xD800 && cp < 0xDC00 && i + 6 <= end && d[i] == '\\' && d[i + 1] == 'u') {
          const int lo = jl_hex4(d, i + 2);
          if (lo < 0) return -1;
          if (lo >= 0xDC00 && lo < 0xE000) {
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
            i += 6;
          }
        }
        if (cp < 0x80) {
          put((unsigned)cp);
        } else if (cp < 0x800) {
          put(0xC0u | (unsigned)(cp >> 6));
          put(0x80u | (unsigned)(cp & 0x3F));
        } else if (cp < 0x10000) {
          put(0xE0u | (unsigned)(cp >> 12));
          put(0x80u | (unsigned)(cp >> 6 & 0x3F));
          put(0x80u | (unsigned)(cp & 0x3F));
        } else {
          put(0xF0u | (unsigned)(cp >> 18));
          put(0x80u | (unsigned)(cp >> 12 & 0x3F));
          put(0x80u | (unsigned)(cp >> 6 & 0x3F));
          put(0x80u | (unsigned)(cp & 0x3F));
        }
        continue;
      }
      unsigned r;
      if (e == '"' || e == '\\' || e == '/') r = e;
      else if (e == 'b') r = 8;
      else if (e == 'f') r = 12;
      else if (e == 'n') r = 10;
      else if (e == 'r') r = 13;
      else if (e == 't') r = 9;
      else return -1;
      put(r);
      continue;
    }
    if (c < 0x80u) {
      put(c);
      ++i;
      continue;
    }
    int n;
    unsigned lo = 0x80u, hi = 0xBFu;
    if (c >= 0xC2u && c <= 0xDFu) n = 1;
    else if (c == 0xE0u) n = 2, lo = 0xA0u;
    else if (c == 0xEDu) n = 2, hi = 0x9Fu;
    else if (c >= 0xE1u && c <= 0xEFu) n = 2;
    else if (c == 0xF0u) n = 3, lo = 0x90u;
    else if (c >= 0xF1u && c <= 0xF3u) n = 3;
    else if (c == 0xF4u) n = 3, hi = 0x8Fu;
    else return -1;
    if (i + n >= end) return -1;
    const unsigned c1 = d[i + 1];
    if (c1 < lo || c1 > hi) return -1;
    for (int k = 2; k <= n; ++k)
      if ((d[i + k] & 0xC0u) != 0x80u) return -1;
    for (int k = 0; k <= n; ++k) put(d[i + k]);
    i += n + 1;
  }
}

// The number literal at d[q]: -?(0|[1-9][0-9]*)(\.[0-9]+)? of at most 18
// digits, followed inside the line by a blank, ',' or '}'. digits: all its
// digits as one integer; frac: how many of them follow the point (-1: none
// and no point). False: not vouched for.
__device__ bool jl_number(const uint8_t *d, long q, long end, bool &neg, long long &digits, int &nd,
                          int &frac) {
  long i = q;
  neg = false;
  digits = 0;
  nd = 0;
  frac = -1;
  if (i < end && d[i] == '-') neg = true, ++i;
  if (i >= end || !jl_digit(d[i])) return false;
  if (d[i] == '0') {
    nd = 1;
    ++i;
  } else {
    while (i < end && jl_digit(d[i])) {
      if (++nd > 18) return false;
      digits = digits * 10 + (long long)(d[i] - '0');
      ++i;
    }
  }
  if (i < end && d[i] == '.') {
    ++i;
    frac = 0;
    while (i < end && jl_digit(d[i])) {
      if (++nd > 18) return false;
      digits = digits * 10 + (long long)(d[i] - '0');
      ++frac;
      ++i;
    }
    if (frac == 0) return false;
  }
  return jl_ends(d, i, end);
}

__device__ __forceinline__ bool jl_word(const uint8_t *d, long q, long end, const char *w, int len) {
  if (q + len > end) return false;
  for (int k = 0; k < len; ++k)
    if (d[q + k] != (uint8_t)w[k]) return false;
  return true;
}

// Bit s of the result: the key d[kbeg, kbeg + klen) is key s of the eight.
__device__ unsigned jl_match_keys(const JsonlParams &P, long kbeg, int klen) {
  const uint8_t *d = P.data;
  unsigned m = 0;
  if (klen == 7 && jl_word(d, kbeg, kbeg + klen, "user_id", 7)) m |= 1u;
  if (klen == 6 && jl_word(d, kbeg, kbeg + klen, "rating", 6)) m |= 4u;
  if (klen == 12 && jl_word(d, kbeg, kbeg + klen, "helpful_vote", 12)) m |= 8u;
  if (klen == 17 && jl_word(d, kbeg, kbeg + klen, "verified_purchase", 17)) m |= 16u;
  if (klen == 9 && jl_word(d, kbeg, kbeg + klen, "timestamp", 9)) m |= 32u;
  if (klen == 5 && jl_word(d, kbeg, kbeg + klen, "title", 5)) m |= 64u;
  if (klen == 4 && jl_word(d, kbeg, kbeg + klen, "text", 4)) m |= 128u;
  if (klen == P.item_key_len) {
    bool same = true;
    for (int k = 0; k < klen; ++k) same &= d[kbeg + k] == P.item_key[k];
    if (same) m |= 2u;
  }
  return m;
}

// Line ln of the chunk, clamped into the data.
__device__ __forceinline__ void jl_line(const JsonlParams &P, long ln, long &beg, long &end) {
  end = jl_clamp((long)P.line_end[ln], 0, (long)P.n_bytes);
  beg = ln ? jl_clamp((long)P.line_end[ln - 1] + 1, 0, end) : 0;
}

__global__ __launch_bounds__(64 * JL_WAVES) void jsonl_scan_kernel(JsonlParams P) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * JL_WAVES + (threadIdx.x >> 6);
  const long n_waves = (long)gridDim.x * JL_WAVES;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint8_t *d = P.data;
  long long n_blank = 0, n_skipped = 0, n_kept = 0, n_flagged = 0;
  for (long ln = wave; ln < P.n_lines; ln += n_waves) {
    long beg, end;
    jl_line(P, ln, beg, end);
    // carried over a step edge (wave-uniform)
    bool flag = false, esc_carry = false, in_str = false, closed = false, seen = false;
    int depth = 0;
    int vp[8];   // the value's first byte per key, relative to beg; -1: the key is missing
#pragma unroll
    for (int s = 0; s < 8; ++s) vp[s] = -1;
    for (long base = beg; base < end; base += 64) {
      const long p = base + lane;
      const bool in = p < end;
      const unsigned b = in ? d[p] : 0x20u;
      const unsigned long long BS = __ballot(b == '\\'), QQ = __ballot(b == '"');
      // bytes after an unescaped backslash
      unsigned long long escd = 0, m = BS;
      if (esc_carry) escd = 1ull, m &= ~1ull;
      esc_carry = false;
      while (m) {   // wave-uniform: one turn per escape
        const int i = __ffsll((long long)m) - 1;
        if (i == 63) {
          esc_carry = true;
          break;
        }
        escd |= 2ull << i;
        m &= ~(3ull << i);
      }
      const unsigned long long Q = QQ & ~escd;
      unsigned long long S = Q;   // inclusive prefix xor: 1 from an opening quote to before the closing
      S ^= S << 1;
      S ^= S << 2;
      S ^= S << 4;
      S ^= S << 8;
      S ^= S << 16;
      S ^= S << 32;
      if (in_str) S = ~S;
      in_str = (S >> 63) != 0ull;
      const bool out = ((~S & ~Q) >> lane & 1ull) != 0ull;   // outside strings, not a quote
      const bool closer = out && (b == '}' || b == ']');
      const unsigned long long OP = __ballot(out && (b == '{' || b == '[')), CL = __ballot(closer);
      const int d_before = depth + __popcll(OP & below) - __popcll(CL & below);
      const unsigned long long NB = __ballot(in && !jl_blank(b));
      bool bad = (b < 0x20u && !(out && b == '\t')) || (out && b == '\\');
      if (!seen && NB) {
        seen = true;
        if (__shfl(b, __ffsll((long long)NB) - 1) != '{') flag = true;
      }
      const unsigned long long ZC = __ballot(closer && d_before == 1);
      if (closed) {
        if (NB) flag = true;
      } else if (ZC) {
        const int i = __ffsll((long long)ZC) - 1;
        if (__shfl(b, i) != '}') flag = true;
        if (i < 63 && (NB >> (i + 1))) flag = true;
        closed = true;
      }
      const bool colon = in && out && b == ':' && d_before == 1;
      unsigned match = 0;
      int vstart = -1;
      if (colon) {
        long q = p - 1;
        while (q >= beg && jl_blank(d[q])) --q;
        if (q < beg || d[q] != '"') {
          bad = true;
        } else {
          const long kend = q;
          --q;
          while (q >= beg && d[q] != '"') {
            if (d[q] == '\\') bad = true;
            --q;
          }
          if (q < beg || (q > beg && d[q - 1] == '\\')) bad = true;
          if (!bad) {
            match = jl_match_keys(P, q + 1, (int)(kend - q - 1));
            long v = p + 1;
            while (v < end && jl_blank(d[v])) ++v;
            vstart = (int)(v - beg);
          }
        }
      }
      if (__ballot(colon)) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const unsigned long long M = __ballot((match >> s & 1u) != 0u);
          if (M) vp[s] = __shfl(vstart, 63 - __clzll((long long)M));
        }
      }
      if (__ballot(bad)) flag = true;
      depth += __popcll(OP) - __popcll(CL);
    }
    if (in_str || depth != 0 || !closed) flag = true;

    // lanes 0 .. 7: one value each. code 0: present, 1: null or missing, 2: not vouched for
    int code = 1, pos = -1;
    long long val = 0;
    if (seen && !flag && lane < 8) {
      int v = -1;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (lane == s) v = vp[s];
      const long q = beg + v;
      if (v >= 0) {
        if (q >= end) {
          code = 2;
        } else if (d[q] == 'n') {
          code = jl_word(d, q, end, "null", 4) && jl_ends(d, q + 4, end) ? 1 : 2;
        } else if (lane < 2 || lane >= 6) {          // the ids, title, text: a string
          long after = end;
          const long size = d[q] == '"' ? jl_string(d, q, end, nullptr, 0, &after) : -1;
          if (size < 0 || !jl_ends(d, after, end)) code = 2;
          else if (size == 0 && lane < 2) code = 1;  // an empty id skips the record
          else code = 0, val = size, pos = (int)q;
        } else if (lane == 4) {                      // verified_purchase
          if (jl_word(d, q, end, "true", 4) && jl_ends(d, q + 4, end)) code = 0, val = 1;
          else if (jl_word(d, q, end, "false", 5) && jl_ends(d, q + 5, end)) code = 0, val = 0;
          else code = 2;
        } else {
          bool neg;
          long long digits;
          int nd, frac;
          if (!jl_number(d, q, end, neg, digits, nd, frac)) {
            code = 2;
          } else if (lane == 2) {                    // rating
            if (nd > 15 || (neg && digits == 0)) {
              code = 2;
            } else {
              double p10 = 1.0;
              for (int k = 0; k < frac; ++k) p10 *= 10.0;   // exact: frac <= 15
              double x = (double)digits;                    // exact: below 10^15
              if (frac > 0) x = x / p10;                    // one correctly rounded division
              code = 0;
              val = __double_as_longlong(neg ? -x : x);
            }
          } else if (frac >= 0) {                    // an integer is read: no float literal
            code = 2;
          } else {
            const long long x = neg ? -digits : digits;
            if (lane == 3 && (x > 2147483647LL || x < -2147483648LL)) code = 2;
            else code = 0, val = x;
          }
        }
      }
    }
    const unsigned long long FL = __ballot(code == 2), AB = __ballot(code == 1);
    int status;
    if (!seen) status = JL_BLANK;
    else if (flag || FL) status = JL_FLAGGED;
    else if (AB & 7ull) status = JL_SKIPPED;       // user id, item id or rating
    else status = JL_KEPT;
    n_blank += status == JL_BLANK;
    n_skipped += status == JL_SKIPPED;
    n_kept += status == JL_KEPT;
    n_flagged += status == JL_FLAGGED;
    // lane s holds key s: each writes its own column
    const bool kept = status == JL_KEPT;
    if (lane == 0) P.status[ln] = (uint8_t)status;
    if (lane == 2) P.rating[ln] = kept ? (float)__longlong_as_double(val) : 0.f;
    if (lane == 3) P.helpful_vote[ln] = kept ? (int)val : 0;
    if (lane == 4) P.verified[ln] = kept && val ? 1 : 0;
    if (lane == 5) {
      P.timestamp[ln] = kept ? val : 0;
      P.ts_valid[ln] = kept && code == 0 ? 1 : 0;
    }
    if (lane < 2 || lane == 6 || lane == 7) {
      const int slot = lane < 2 ? lane : lane - 4;
      P.sizes[ln * 4 + slot] = kept ? (int)val : 0;
      P.spos[ln * 4 + slot] = kept ? pos : -1;
    }
  }
  if (lane == 0) {
    unsigned long long *t = reinterpret_cast<unsigned long long *>(P.totals);
    if (n_blank) atomicAdd(t, (unsigned long long)n_blank);
    if (n_skipped) atomicAdd(t + 1, (unsigned long long)n_skipped);
    if (n_kept) atomicAdd(t + 2, (unsigned long long)n_kept);
    if (n_flagged) atomicAdd(t + 3, (unsigned long long)n_flagged);
  }
}

// What line i adds to scan `which`: 0 a record, 1 / 2 its user / item id
// bytes, 3 its text bytes (title + " " + text; a host-supplied line's text is
// whole in slot 2). i = n: the scans' totals land there.
struct JlSize {
  const uint8_t *status;
  const int *sizes;
  long n;
  int which;
  __host__ __device__ __forceinline__ long long at(long i, int slot) const {
    const int v = sizes[i * 4 + slot];
    return v > 0 ? v : 0;
  }
  __host__ __device__ __forceinline__ long long operator()(long i) const {
    if (i < 0 || i >= n) return 0;
    const int s = status[i];
    if (s != JL_KEPT && s != JL_HOST) return 0;
    if (which == 0) return 1;
    if (which < 3) return at(i, which - 1);
    return s == JL_HOST ? at(i, 2) : at(i, 2) + 1 + at(i, 3);
  }
};
typedef hipcub::TransformInputIterator<long long, JlSize, hipcub::CountingInputIterator<long>>
    JlSizeIter;

__global__ __launch_bounds__(64 * JL_WAVES) void jsonl_write_kernel(JsonlParams P) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * JL_WAVES + (threadIdx.x >> 6);
  const long n_waves = (long)gridDim.x * JL_WAVES;
  const long stride = (long)P.n_lines + 1;
  const long caps[3] = {(long)P.user_bytes, (long)P.item_bytes, (long)P.text_bytes};
  for (long ln = wave; ln < P.n_lines; ln += n_waves) {
    const int status = P.status[ln];
    if (status != JL_KEPT && status != JL_HOST) continue;
    const long rec = (long)P.offs[ln];
    if (rec < 0 || rec >= P.n_records) continue;
    const long uo = jl_clamp((long)P.offs[stride + ln], 0, caps[0]);
    const long io = jl_clamp((long)P.offs[2 * stride + ln], 0, caps[1]);
    const long to = jl_clamp((long)P.offs[3 * stride + ln], 0, caps[2]);
    if (lane == 0) {
      P.out_rating[rec] = P.rating[ln];
      P.out_helpful[rec] = P.helpful_vote[ln];
      P.out_verified[rec] = P.verified[ln];
      P.out_timestamp[rec] = P.timestamp[ln];
      P.out_ts_valid[rec] = P.ts_valid[ln];
      P.user_off[rec] = uo;
      P.item_off[rec] = io;
      P.text_off[rec] = to;
    }
    if (status == JL_HOST) {   // the host's bytes, copied by the whole wave
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const long size = P.sizes[ln * 4 + s], from = P.spos[ln * 4 + s];
        uint8_t *dst = s == 0 ? P.user_data + uo : (s == 1 ? P.item_data + io : P.text_data + to);
        const long room = caps[s] - (s == 0 ? uo : (s == 1 ? io : to));
        if (size <= 0 || from < 0 || from + size > P.side_bytes) continue;
        for (long k = lane; k < size && k < room; k += 64) dst[k] = P.side[from + k];
      }
      continue;
    }
    long beg, end;
    jl_line(P, ln, beg, end);
    if (lane < 4) {
      const long q = P.spos[ln * 4 + lane];
      const long title = P.sizes[ln * 4 + 2] > 0 ? P.sizes[ln * 4 + 2] : 0;
      uint8_t *dst = lane == 0 ? P.user_data + uo : (lane == 1 ? P.item_data + io : P.text_data + to);
      long room = lane == 0 ? caps[0] - uo : (lane == 1 ? caps[1] - io : caps[2] - to);
      if (lane == 2 && title < room) dst[title] = ' ';
      if (lane == 3) {
        dst += title + 1;
        room -= title + 1;
      }
      if (q >= beg && q < end && P.data[q] == '"' && room > 0)
        (void)jl_string(P.data, q, end, dst, room);
    }
  }
}

// ---------------------------------------------------------------------------
// numbering
// ---------------------------------------------------------------------------
struct IdsParams {
  long n;
  const uint8_t *data;
  const long long *offsets;
  long data_bytes;
  unsigned long long hash_mask;
};

__device__ __forceinline__ void ids_range(const IdsParams &P, long r, long &beg, long &end) {
  end = jl_clamp((long)P.offsets[r + 1], 0, P.data_bytes);
  beg = jl_clamp((long)P.offsets[r], 0, end);
}

__global__ __launch_bounds__(256) void ids_hash_kernel(IdsParams P, unsigned long long *keys,
                                                       uint32_t *vals) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= P.n) return;
  long beg, end;
  ids_range(P, r, beg, end);
  unsigned long long h = 0xcbf29ce484222325ull;   // FNV-1a, 64 bits
  for (long p = beg; p < end; ++p) h = (h ^ (unsigned long long)P.data[p]) * 0x100000001b3ull;
  h ^= h >> 29;   // finaliser: the high bits reach the low ones a narrow mask keeps
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  keys[r] = h & P.hash_mask;
  vals[r] = (uint32_t)r;
}

// One lane per sorted slot: head[j] = 1 where a run of equal hashes begins; a
// slot whose string differs from its left neighbour's under an equal hash
// counts in totals[1]. first[r] = 1 for the record of a head: the sort is
// stable, so that is the run's first record in file order.
__global__ __launch_bounds__(256) void ids_verify_kernel(IdsParams P,
                                                         const unsigned long long *keys,
                                                         const uint32_t *vals, int *head,
                                                         int *first, long long *totals) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.n) return;
  const long r = vals[j];
  bool opens = j == 0 || keys[j] != keys[j - 1];
  if (r >= P.n) opens = false;   // never, after the sort
  if (!opens && r < P.n) {
    const long l = vals[j - 1];
    bool differ = l >= P.n;
    if (!differ) {
      long b0, e0, b1, e1;
      ids_range(P, r, b0, e0);
      ids_range(P, l, b1, e1);
      differ = e0 - b0 != e1 - b1;
      for (long k = 0; !differ && k < e0 - b0; ++k) differ = P.data[b0 + k] != P.data[b1 + k];
    }
    if (differ) atomicAdd(reinterpret_cast<unsigned long long *>(totals) + 1, 1ull);
  }
  head[j] = opens ? 1 : 0;
  if (opens) first[r] = 1;
}

// run[j]: the inclusive scan of head. The record of run k's head.
__global__ __launch_bounds__(256) void ids_heads_kernel(long n, const uint32_t *vals,
                                                        const int *head, const int *run,
                                                        int *run_rec) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n || !head[j]) return;
  const long k = (long)run[j] - 1;
  if (k >= 0 && k < n) run_rec[k] = (int)vals[j];
}

// rank[r]: the exclusive scan of first in record order, the id of a string
// first seen at r. ids[record] = the id of its run; first_rec[id] = r.
__global__ __launch_bounds__(256) void ids_assign_kernel(long n, const uint32_t *vals,
                                                         const int *run, const int *run_rec,
                                                         const int *first, const int *rank,
                                                         int *ids, int *first_rec,
                                                         long long *totals) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const long r = vals[j], k = (long)run[j] - 1;
  if (r < n && k >= 0 && k < n) {
    const long h = run_rec[k];
    if (h >= 0 && h < n) ids[r] = rank[h];
  }
  if (first[j]) {   // j as a record here
    const long id = rank[j];
    if (id >= 0 && id < n) first_rec[id] = (int)j;
  }
  if (j == n - 1) totals[0] = (long long)rank[j] + (first[j] ? 1 : 0);
}

// The length of id k's string, that of record first_rec[k]; 0 past n_ids.
struct IdLen {
  const int *first_rec;
  const long long *offsets;
  long n_ids, n;
  __host__ __device__ __forceinline__ long long operator()(long k) const {
    if (k < 0 || k >= n_ids) return 0;
    const long r = first_rec[k];
    if (r < 0 || r >= n) return 0;
    const long long len = offsets[r + 1] - offsets[r];
    return len > 0 ? len : 0;
  }
};
typedef hipcub::TransformInputIterator<long long, IdLen, hipcub::CountingInputIterator<long>>
    IdLenIter;

__global__ __launch_bounds__(64 * JL_WAVES) void ids_table_kernel(IdsParams P, long n_ids,
                                                                  const int *first_rec,
                                                                  const long long *tab_off,
                                                                  uint8_t *tab_data,
                                                                  long tab_bytes) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * JL_WAVES + (threadIdx.x >> 6);
  const long n_waves = (long)gridDim.x * JL_WAVES;
  for (long k = wave; k < n_ids; k += n_waves) {
    const long r = first_rec[k];
    if (r < 0 || r >= P.n) continue;
    long beg, end;
    ids_range(P, r, beg, end);
    const long to = jl_clamp((long)tab_off[k], 0, tab_bytes);
    for (long i = lane; i < end - beg && to + i < tab_bytes; i += 64) tab_data[to + i] = P.data[beg + i];
  }
}

static unsigned jl_wave_blocks(long n) {
  const long b = (n + JL_WAVES - 1) / JL_WAVES;
  return (unsigned)(b < 1 ? 1 : (b < JL_MAX_BLOCKS ? b : JL_MAX_BLOCKS));
}

static int jl_check(const char *fn, const bbgr_jsonl_args *a, bool lines) {
  BBGR_REQUIRE_IN(fn, a, "null args");
  BBGR_REQUIRE_IN(fn, a->n_bytes >= 0 && a->n_bytes < JL_N_MAX,
                  "n_bytes out of range (must be < 2^31 - 1)");
  if (a->n_bytes > 0) {
    BBGR_REQUIRE_IN(fn, a->data, "null data");
    BBGR_REQUIRE_IN(fn, a->totals, "null totals");
  }
  if (lines) {
    BBGR_REQUIRE_IN(fn, a->n_lines >= 0 && a->n_lines <= a->n_bytes,
                    "n_lines out of range (at most n_bytes)");
    if (a->n_lines > 0) BBGR_REQUIRE_IN(fn, a->line_end, "null line_end");
  }
  return BBGR_OK;
}

static int jl_check_scan(const char *fn, const bbgr_jsonl_args *a) {
  if (int rc = jl_check(fn, a, true)) return rc;
  if (a->n_lines > 0) {
    BBGR_REQUIRE_IN(fn, a->status, "null status");
    BBGR_REQUIRE_IN(fn, a->rating, "null rating");
    BBGR_REQUIRE_IN(fn, a->helpful_vote, "null helpful_vote");
    BBGR_REQUIRE_IN(fn, a->verified, "null verified");
    BBGR_REQUIRE_IN(fn, a->timestamp, "null timestamp");
    BBGR_REQUIRE_IN(fn, a->ts_valid, "null ts_valid");
    BBGR_REQUIRE_IN(fn, a->sizes, "null sizes");
    BBGR_REQUIRE_IN(fn, a->spos, "null spos");
  }
  return BBGR_OK;
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_jsonl_count(const bbgr_jsonl_args *a, bbgr_stream_t stream) {
  static const char *fn = "bbgr_jsonl_count";
  if (int rc = jl_check(fn, a, false)) return rc;
  if (a->n_bytes == 0) return BBGR_OK;
  hipStream_t st = as_stream(stream);
  const long n_tiles = ((long)a->n_bytes + JL_TILE - 1) / JL_TILE;
  BBGR_HIP(hipMemsetAsync(a->totals, 0, 4 * sizeof(int64_t), st));
  hipLaunchKernelGGL(jsonl_tile_kernel<false>, dim3(jl_wave_blocks(n_tiles)), dim3(64 * JL_WAVES), 0,
                     st, (long)a->n_bytes, a->data, n_tiles, (int *)nullptr, (const int *)nullptr, 0L,
                     (int *)nullptr, reinterpret_cast<long long *>(a->totals));
  BBGR_LAUNCHED("jsonl_tile_kernel<count>");
  return BBGR_OK;
}

extern "C" int bbgr_jsonl_lines(const bbgr_jsonl_args *a, void *workspace, size_t *workspace_bytes,
                                bbgr_stream_t stream) {
  static const char *fn = "bbgr_jsonl_lines";
  if (int rc = jl_check(fn, a, true)) return rc;
  const long n_tiles = ((long)a->n_bytes + JL_TILE - 1) / JL_TILE;
  const size_t t_scan = hcub::exclusive_sum_temp<const int *, int *>((int)n_tiles);
  Carver C;
  const size_t off_count = C.take_n<int>((size_t)n_tiles), off_off = C.take_n<int>((size_t)n_tiles);
  const size_t off_tmp = C.take(t_scan);
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query || a->n_lines == 0) return rc;
  hipStream_t st = as_stream(stream);
  int *tile_count = ws_at<int>(workspace, off_count);
  int *tile_off = ws_at<int>(workspace, off_off);
  const dim3 grid(jl_wave_blocks(n_tiles)), block(64 * JL_WAVES);
  hipLaunchKernelGGL(jsonl_tile_kernel<false>, grid, block, 0, st, (long)a->n_bytes, a->data, n_tiles,
                     tile_count, (const int *)nullptr, 0L, (int *)nullptr, (long long *)nullptr);
  BBGR_LAUNCHED("jsonl_tile_kernel<count>");
  BBGR_HIP(hcub::exclusive_sum(ws_at<char>(workspace, off_tmp), t_scan, (const int *)tile_count,
                               tile_off, (int)n_tiles, st));
  hipLaunchKernelGGL(jsonl_tile_kernel<true>, grid, block, 0, st, (long)a->n_bytes, a->data, n_tiles,
                     (int *)nullptr, (const int *)tile_off, (long)a->n_lines, a->line_end,
                     (long long *)nullptr);
  BBGR_LAUNCHED("jsonl_tile_kernel<scatter>");
  return BBGR_OK;
}

extern "C" int bbgr_jsonl_scan(const bbgr_jsonl_args *a, bbgr_stream_t stream) {
  static const char *fn = "bbgr_jsonl_scan";
  if (int rc = jl_check_scan(fn, a)) return rc;
  BBGR_REQUIRE_IN(fn, a->item_key_len >= 1 && a->item_key_len <= 255,
                  "item_key_len out of range (1 .. 255)");
  if (a->n_lines == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, a->item_key, "null item_key");
  hipStream_t st = as_stream(stream);
  BBGR_HIP(hipMemsetAsync(a->totals, 0, 4 * sizeof(int64_t), st));
  hipLaunchKernelGGL(jsonl_scan_kernel, dim3(jl_wave_blocks((long)a->n_lines)), dim3(64 * JL_WAVES),
                     0, st, *a);
  BBGR_LAUNCHED("jsonl_scan_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_jsonl_offsets(const bbgr_jsonl_args *a, void *workspace,
                                  size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_jsonl_offsets";
  if (int rc = jl_check_scan(fn, a)) return rc;
  BBGR_REQUIRE_IN(fn, a->offs, "null offs");
  const long n = (long)a->n_lines;
  const size_t t_scan = hcub::exclusive_sum_temp<JlSizeIter, long long *>(
      (int)(n + 1), nullptr,
      JlSizeIter(hipcub::CountingInputIterator<long>(0), JlSize{nullptr, nullptr, n, 0}));
  bool query;
  int rc = take_workspace(fn, align_up(t_scan), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  hipStream_t st = as_stream(stream);
  for (int which = 0; which < 4; ++which) {
    const JlSizeIter in(hipcub::CountingInputIterator<long>(0),
                        JlSize{a->status, a->sizes, n, which});
    BBGR_HIP(hcub::exclusive_sum(
        workspace, t_scan, in,
        reinterpret_cast<long long *>(a->offs) + (size_t)which * (size_t)(n + 1), (int)(n + 1), st));
  }
  return BBGR_OK;
}

extern "C" int bbgr_jsonl_write(const bbgr_jsonl_args *a, bbgr_stream_t stream) {
  static const char *fn = "bbgr_jsonl_write";
  if (int rc = jl_check_scan(fn, a)) return rc;
  BBGR_REQUIRE_IN(fn, a->n_records >= 0 && a->n_records <= a->n_lines,
                  "n_records out of range (at most n_lines)");
  BBGR_REQUIRE_IN(fn, a->user_bytes >= 0 && a->user_bytes < JL_N_MAX, "user_bytes out of range");
  BBGR_REQUIRE_IN(fn, a->item_bytes >= 0 && a->item_bytes < JL_N_MAX, "item_bytes out of range");
  BBGR_REQUIRE_IN(fn, a->text_bytes >= 0 && a->text_bytes < 2 * JL_N_MAX, "text_bytes out of range");
  BBGR_REQUIRE_IN(fn, a->side_bytes >= 0 && a->side_bytes < JL_N_MAX, "side_bytes out of range");
  BBGR_REQUIRE_IN(fn, a->side_bytes == 0 || a->side, "null side");
  if (a->n_records == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, a->offs, "null offs");
  BBGR_REQUIRE_IN(fn, a->out_rating && a->out_helpful && a->out_verified && a->out_timestamp &&
                          a->out_ts_valid, "null output column");
  BBGR_REQUIRE_IN(fn, a->user_off && a->item_off && a->text_off, "null output offsets");
  BBGR_REQUIRE_IN(fn, a->user_data && a->item_data && a->text_data, "null output bytes");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(jsonl_write_kernel, dim3(jl_wave_blocks((long)a->n_lines)), dim3(64 * JL_WAVES),
                     0, st, *a);
  BBGR_LAUNCHED("jsonl_write_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_ids_number(int64_t n, const uint8_t *data, const int64_t *offsets,
                               int64_t data_bytes, uint64_t hash_mask, int32_t *ids,
                               int32_t *first_rec, int64_t *totals, void *workspace,
                               size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_ids_number";
  BBGR_REQUIRE_IN(fn, n >= 0 && n < JL_N_MAX, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, data_bytes >= 0, "data_bytes < 0");
  if (n > 0) {
    BBGR_REQUIRE_IN(fn, data, "null data");
    BBGR_REQUIRE_IN(fn, offsets, "null offsets");
    BBGR_REQUIRE_IN(fn, ids, "null ids");
    BBGR_REQUIRE_IN(fn, first_rec, "null first_rec");
    BBGR_REQUIRE_IN(fn, totals, "null totals");
  }
  size_t t_sort = 0, t_scan = 0;
  if (n > 0) {
    t_sort = hcub::sort_pairs_temp<unsigned long long, uint32_t>((int)n, 0, 64);
    t_scan = hcub::inclusive_sum_temp<const int *, int *>((int)n);
  }
  const size_t temp = t_sort > t_scan ? t_sort : t_scan;
  const size_t u = (size_t)n;
  Carver C;
  const size_t off_k1 = C.take_n<unsigned long long>(u), off_k2 = C.take_n<unsigned long long>(u);
  const size_t off_v1 = C.take_n<uint32_t>(u), off_v2 = C.take_n<uint32_t>(u);
  const size_t off_head = C.take_n<int>(u), off_run = C.take_n<int>(u);
  const size_t off_run_rec = C.take_n<int>(u), off_first = C.take_n<int>(u);
  const size_t off_rank = C.take_n<int>(u), off_tmp = C.take(temp);
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query || n == 0) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long *k1 = ws_at<unsigned long long>(workspace, off_k1);
  unsigned long long *k2 = ws_at<unsigned long long>(workspace, off_k2);
  uint32_t *v1 = ws_at<uint32_t>(workspace, off_v1), *v2 = ws_at<uint32_t>(workspace, off_v2);
  int *head = ws_at<int>(workspace, off_head), *run = ws_at<int>(workspace, off_run);
  int *run_rec = ws_at<int>(workspace, off_run_rec);
  int *first = ws_at<int>(workspace, off_first), *rank = ws_at<int>(workspace, off_rank);
  void *tmp = ws_at<char>(workspace, off_tmp);
  const IdsParams P{(long)n, data, reinterpret_cast<const long long *>(offsets), (long)data_bytes,
                    hash_mask ? hash_mask : ~0ull};
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  BBGR_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
  BBGR_HIP(hipMemsetAsync(first, 0, sizeof(int) * (size_t)n, st));
  BBGR_HIP(hipMemsetAsync(run_rec, 0, sizeof(int) * (size_t)n, st));
  hipLaunchKernelGGL(ids_hash_kernel, grid, block, 0, st, P, k1, v1);
  BBGR_LAUNCHED("ids_hash_kernel");
  BBGR_HIP(hcub::sort_pairs(tmp, temp, (const unsigned long long *)k1, k2, (const uint32_t *)v1,
                            v2, (int)n, 0, 64, st));
  hipLaunchKernelGGL(ids_verify_kernel, grid, block, 0, st, P, (const unsigned long long *)k2,
                     (const uint32_t *)v2, head, first, reinterpret_cast<long long *>(totals));
  BBGR_LAUNCHED("ids_verify_kernel");
  BBGR_HIP(hcub::inclusive_sum(tmp, temp, (const int *)head, run, (int)n, st));
  BBGR_HIP(hcub::exclusive_sum(tmp, temp, (const int *)first, rank, (int)n, st));
  hipLaunchKernelGGL(ids_heads_kernel, grid, block, 0, st, (long)n, (const uint32_t *)v2,
                     (const int *)head, (const int *)run, run_rec);
  BBGR_LAUNCHED("ids_heads_kernel");
  hipLaunchKernelGGL(ids_assign_kernel, grid, block, 0, st, (long)n, (const uint32_t *)v2,
                     (const int *)run, (const int *)run_rec, (const int *)first, (const int *)rank,
                     ids, first_rec, reinterpret_cast<long long *>(totals));
  BBGR_LAUNCHED("ids_assign_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_ids_table(int64_t n_ids, const int32_t *first_rec, int64_t n,
                              const uint8_t *data, const int64_t *offsets, int64_t data_bytes,
                              int64_t *tab_offsets, uint8_t *tab_data, int64_t tab_bytes,
                              void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_ids_table";
  BBGR_REQUIRE_IN(fn, n >= 0 && n < JL_N_MAX, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, n_ids >= 0 && n_ids <= n, "n_ids out of range (at most n)");
  BBGR_REQUIRE_IN(fn, data_bytes >= 0, "data_bytes < 0");
  BBGR_REQUIRE_IN(fn, tab_bytes >= 0 && tab_bytes <= data_bytes,
                  "tab_bytes out of range (at most data_bytes)");
  BBGR_REQUIRE_IN(fn, tab_offsets, "null tab_offsets");
  if (n_ids > 0) {
    BBGR_REQUIRE_IN(fn, first_rec, "null first_rec");
    BBGR_REQUIRE_IN(fn, data, "null data");
    BBGR_REQUIRE_IN(fn, offsets, "null offsets");
  }
  const IdLenIter in(hipcub::CountingInputIterator<long>(0),
                     IdLen{first_rec, reinterpret_cast<const long long *>(offsets), (long)n_ids,
                           (long)n});
  const size_t t_scan =
      hcub::exclusive_sum_temp<IdLenIter, long long *>((int)(n_ids + 1), nullptr, in);
  bool query;
  int rc = take_workspace(fn, align_up(t_scan), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  hipStream_t st = as_stream(stream);
  if (!tab_data) {   // the offsets alone: tab_offsets[n_ids] sizes the table
    BBGR_HIP(hcub::exclusive_sum(workspace, t_scan, in, reinterpret_cast<long long *>(tab_offsets),
                                 (int)(n_ids + 1), st));
    return BBGR_OK;
  }
  if (n_ids == 0 || tab_bytes == 0) return BBGR_OK;
  const IdsParams P{(long)n, data, reinterpret_cast<const long long *>(offsets), (long)data_bytes,
                    ~0ull};
  hipLaunchKernelGGL(ids_table_kernel, dim3(jl_wave_blocks((long)n_ids)), dim3(64 * JL_WAVES), 0, st,
                     P, (long)n_ids, first_rec, reinterpret_cast<const long long *>(tab_offsets),
                     tab_data, (long)tab_bytes);
  BBGR_LAUNCHED("ids_table_kernel");
  return BBGR_OK;
}
