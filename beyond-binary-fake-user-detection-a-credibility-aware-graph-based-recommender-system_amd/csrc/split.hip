// The md5 train / val / test split of review records
// (build_graph_from_jsonl, lighgcn_cu_pop.py:227-303): which records are
// positive, the first-appearance numbering of users and items among them, and
// the bucket of every kept pair by the first 32 bits of md5("{uid}|{iid}").
//
// bbgr_md5_pair_hash: one record per thread. The message is never built in
// memory: a 64-byte block is sixteen words fetched straight from the two id
// pools. A word that lies whole inside one id is one 4-byte load at the id's
// own (unaligned) address; only the words that hold the separator, the 0x80
// pad or an id's ragged end are put together byte by byte. With the dataset's
// ids (28 + 1 + 10 bytes) that is 8 word loads and 2 assembled words of 16.
// The sixteen words and the state stay in registers: every index below is a
// literal, the 64 steps are written out.
//
// bbgr_split_edges: integer work only. An unsigned atomicMin of the record
// index per id finds every id's first positive record (order-free: the min is
// the same however the atomics land); a record is "first" when it is that
// minimum. Five 0/1 flags per record (train, val, test, first of its user,
// first of its item) are then scanned exclusively: per tile of SPLIT_TILE
// records a count, one workgroup scans the tile counts, and two scatter
// launches rank every record inside its tile by wave ballots. Ranks follow the
// record index, so every output is in file order and two calls give the same
// bits.
//
// Measured at 1M and 50M records in DESIGN 4e (tools/split_bench.py).
#include "common.h"

#include <limits.h>
#include <string.h>

namespace bbgr {

constexpr int SPLIT_ROUNDS = 8;                    // records per thread of a tile
constexpr int SPLIT_TILE = 256 * SPLIT_ROUNDS;     // records per workgroup: 2048
constexpr int SPLIT_SEGS = 4 * SPLIT_ROUNDS;       // (round, wave) runs of 64 records
constexpr int SPLIT_NC = 5;                        // train, val, test, first-of-user, first-of-item
constexpr unsigned long long SPLIT_THR_MAX = 1ull << 32;

// per-record code (workspace, one byte): 0 not positive, else bucket + 1 in
// bits 0-1, bit 2 first of its user, bit 3 first of its item
constexpr int CODE_FIRST_U = 4, CODE_FIRST_I = 8;

// ---------------------------------------------------------------------------
// md5 (RFC 1321) of user_id + "|" + item_id, first four digest bytes
// ---------------------------------------------------------------------------
struct Md5Msg {
  const uint8_t *u;   // user id bytes
  const uint8_t *v;   // item id bytes
  long ulen;          // bytes of the user id
  long len;           // ulen + 1 + bytes of the item id
};

__host__ __device__ __forceinline__ uint32_t md5_byte(const Md5Msg &m, long q) {
  if (q < m.ulen) return m.u[q];
  if (q == m.ulen) return (uint32_t)'|';
  if (q < m.len) return m.v[q - m.ulen - 1];
  return q == m.len ? 0x80u : 0u;
}

// Message bytes p .. p + 3 as a little-endian word, p a multiple of 4; past the
// message: the 0x80 pad byte, then zeros.
__host__ __device__ __forceinline__ uint32_t md5_word(const Md5Msg &m, long p) {
  uint32_t w;
  if (p + 4 <= m.ulen) {
    memcpy(&w, m.u + p, 4);
    return w;
  }
  if (p > m.ulen && p + 4 <= m.len) {
    memcpy(&w, m.v + (p - m.ulen - 1), 4);
    return w;
  }
  if (p > m.len) return 0u;
  return md5_byte(m, p) | md5_byte(m, p + 1) << 8 | md5_byte(m, p + 2) << 16 |
         md5_byte(m, p + 3) << 24;
}

__host__ __device__ __forceinline__ uint32_t md5_rotl(uint32_t x, int s) {
  return x << s | x >> (32 - s);
}

#define MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, w, k, s) a = b + md5_rotl(a + f(b, c, d) + (w) + k, s)

// int(hexdigest[:8], 16) of md5 over the message: digest bytes 0..3 big-endian.
__host__ __device__ inline uint32_t md5_hash32(const Md5Msg &m) {
  uint32_t a0 = 0x67452301u, b0 = 0xefcdab89u, c0 = 0x98badcfeu, d0 = 0x10325476u;
  const long n_blocks = (m.len + 8) / 64 + 1;   // the 0x80 byte and the 64-bit length fit
  for (long blk = 0; blk < n_blocks; ++blk) {
    const long p = blk * 64;
    const uint32_t w0 = md5_word(m, p), w1 = md5_word(m, p + 4), w2 = md5_word(m, p + 8),
                   w3 = md5_word(m, p + 12), w4 = md5_word(m, p + 16), w5 = md5_word(m, p + 20),
                   w6 = md5_word(m, p + 24), w7 = md5_word(m, p + 28), w8 = md5_word(m, p + 32),
                   w9 = md5_word(m, p + 36), w10 = md5_word(m, p + 40), w11 = md5_word(m, p + 44),
                   w12 = md5_word(m, p + 48), w13 = md5_word(m, p + 52);
    uint32_t w14 = md5_word(m, p + 56), w15 = md5_word(m, p + 60);
    if (blk == n_blocks - 1) {   // the message length in bits, 64-bit little-endian
      const unsigned long long bits = (unsigned long long)m.len * 8ull;
      w14 = (uint32_t)bits;
      w15 = (uint32_t)(bits >> 32);
    }
    uint32_t a = a0, b = b0, c = c0, d = d0;
    MD5_STEP(MD5_F, a, b, c, d, w0, 0xd76aa478u, 7);
    MD5_STEP(MD5_F, d, a, b, c, w1, 0xe8c7b756u, 12);
    MD5_STEP(MD5_F, c, d, a, b, w2, 0x242070dbu, 17);
    MD5_STEP(MD5_F, b, c, d, a, w3, 0xc1bdceeeu, 22);
    MD5_STEP(MD5_F, a, b, c, d, w4, 0xf57c0fafu, 7);
    MD5_STEP(MD5_F, d, a, b, c, w5, 0x4787c62au, 12);
    MD5_STEP(MD5_F, c, d, a, b, w6, 0xa8304613u, 17);
    MD5_STEP(MD5_F, b, c, d, a, w7, 0xfd469501u, 22);
    MD5_STEP(MD5_F, a, b, c, d, w8, 0x698098d8u, 7);
    MD5_STEP(MD5_F, d, a, b, c, w9, 0x8b44f7afu, 12);
    MD5_STEP(MD5_F, c, d, a, b, w10, 0xffff5bb1u, 17);
    MD5_STEP(MD5_F, b, c, d, a, w11, 0x895cd7beu, 22);
    MD5_STEP(MD5_F, a, b, c, d, w12, 0x6b901122u, 7);
    MD5_STEP(MD5_F, d, a, b, c, w13, 0xfd987193u, 12);
    MD5_STEP(MD5_F, c, d, a, b, w14, 0xa679438eu, 17);
    MD5_STEP(MD5_F, b, c, d, a, w15, 0x49b40821u, 22);

    MD5_STEP(MD5_G, a, b, c, d, w1, 0xf61e2562u, 5);
    MD5_STEP(MD5_G, d, a, b, c, w6, 0xc040b340u, 9);
    MD5_STEP(MD5_G, c, d, a, b, w11, 0x265e5a51u, 14);
    MD5_STEP(MD5_G, b, c, d, a, w0, 0xe9b6c7aau, 20);
    MD5_STEP(MD5_G, a, b, c, d, w5, 0xd62f105du, 5);
    MD5_STEP(MD5_G, d, a, b, c, w10, 0x02441453u, 9);
    MD5_STEP(MD5_G, c, d, a, b, w15, 0xd8a1e681u, 14);
    MD5_STEP(MD5_G, b, c, d, a, w4, 0xe7d3fbc8u, 20);
    MD5_STEP(MD5_G, a, b, c, d, w9, 0x21e1cde6u, 5);
    MD5_STEP(MD5_G, d, a, b, c, w14, 0xc33707d6u, 9);
    MD5_STEP(MD5_G, c, d, a, b, w3, 0xf4d50d87u, 14);
    MD5_STEP(MD5_G, b, c, d, a, w8, 0x455a14edu, 20);
    MD5_STEP(MD5_G, a, b, c, d, w13, 0xa9e3e905u, 5);
    MD5_STEP(MD5_G, d, a, b, c, w2, 0xfcefa3f8u, 9);
    MD5_STEP(MD5_G, c, d, a, b, w7, 0x676f02d9u, 14);
    MD5_STEP(MD5_G, b, c, d, a, w12, 0x8d2a4c8au, 20);

    MD5_STEP(MD5_H, a, b, c, d, w5, 0xfffa3942u, 4);
    MD5_STEP(MD5_H, d, a, b, c, w8, 0x8771f681u, 11);
    MD5_STEP(MD5_H, c, d, a, b, w11, 0x6d9d6122u, 16);
    MD5_STEP(MD5_H, b, c, d, a, w14, 0xfde5380cu, 23);
    MD5_STEP(MD5_H, a, b, c, d, w1, 0xa4beea44u, 4);
    MD5_STEP(MD5_H, d, a, b, c, w4, 0x4bdecfa9u, 11);
    MD5_STEP(MD5_H, c, d, a, b, w7, 0xf6bb4b60u, 16);
    MD5_STEP(MD5_H, b, c, d, a, w10, 0xbebfbc70u, 23);
    MD5_STEP(MD5_H, a, b, c, d, w13, 0x289b7ec6u, 4);
    MD5_STEP(MD5_H, d, a, b, c, w0, 0xeaa127fau, 11);
    MD5_STEP(MD5_H, c, d, a, b, w3, 0xd4ef3085u, 16);
    MD5_STEP(MD5_H, b, c, d, a, w6, 0x04881d05u, 23);
    MD5_STEP(MD5_H, a, b, c, d, w9, 0xd9d4d039u, 4);
    MD5_STEP(MD5_H, d, a, b, c, w12, 0xe6db99e5u, 11);
    MD5_STEP(MD5_H, c, d, a, b, w15, 0x1fa27cf8u, 16);
    MD5_STEP(MD5_H, b, c, d, a, w2, 0xc4ac5665u, 23);

    MD5_STEP(MD5_I, a, b, c, d, w0, 0xf4292244u, 6);
    MD5_STEP(MD5_I, d, a, b, c, w7, 0x432aff97u, 10);
    MD5_STEP(MD5_I, c, d, a, b, w14, 0xab9423a7u, 15);
    MD5_STEP(MD5_I, b, c, d, a, w5, 0xfc93a039u, 21);
    MD5_STEP(MD5_I, a, b, c, d, w12, 0x655b59c3u, 6);
    MD5_STEP(MD5_I, d, a, b, c, w3, 0x8f0ccc92u, 10);
    MD5_STEP(MD5_I, c, d, a, b, w10, 0xffeff47du, 15);
    MD5_STEP(MD5_I, b, c, d, a, w1, 0x85845dd1u, 21);
    MD5_STEP(MD5_I, a, b, c, d, w8, 0x6fa87e4fu, 6);
    MD5_STEP(MD5_I, d, a, b, c, w15, 0xfe2ce6e0u, 10);
    MD5_STEP(MD5_I, c, d, a, b, w6, 0xa3014314u, 15);
    MD5_STEP(MD5_I, b, c, d, a, w13, 0x4e0811a1u, 21);
    MD5_STEP(MD5_I, a, b, c, d, w4, 0xf7537e82u, 6);
    MD5_STEP(MD5_I, d, a, b, c, w11, 0xbd3af235u, 10);
    MD5_STEP(MD5_I, c, d, a, b, w2, 0x2ad7d2bbu, 15);
    MD5_STEP(MD5_I, b, c, d, a, w9, 0xeb86d391u, 21);
    a0 += a;
    b0 += b;
    c0 += c;
    d0 += d;
  }
  return a0 << 24 | (a0 & 0xff00u) << 8 | (a0 >> 8 & 0xff00u) | a0 >> 24;
}

#undef MD5_F
#undef MD5_G
#undef MD5_H
#undef MD5_I
#undef MD5_STEP

struct Md5Params {
  long n;
  const int *user;
  const int *item;
  const uint8_t *user_data;
  const long long *user_offsets;
  int n_users;
  const uint8_t *item_data;
  const long long *item_offsets;
  int n_items;
  const uint8_t *keep;
  uint32_t *hash32;
};

// A record whose id lies outside its table is skipped like a masked one (the
// caller checks ids; nothing is read out of bounds either way).
__global__ __launch_bounds__(256) void md5_pair_hash_kernel(Md5Params P) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= P.n) return;
  if (P.keep && !P.keep[e]) return;
  const int u = P.user[e], it = P.item[e];
  if (u < 0 || u >= P.n_users || it < 0 || it >= P.n_items) return;
  const long long ub = P.user_offsets[u], ue = P.user_offsets[u + 1];
  const long long ib = P.item_offsets[it], ie = P.item_offsets[it + 1];
  if (ue < ub || ie < ib) return;
  Md5Msg m;
  m.u = P.user_data + ub;
  m.v = P.item_data + ib;
  m.ulen = (long)(ue - ub);
  m.len = m.ulen + 1 + (long)(ie - ib);
  P.hash32[e] = md5_hash32(m);
}

// ---------------------------------------------------------------------------
// The split
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool split_positive(const bbgr_split_args &A, long e, int u, int it) {
  const bool pos = A.positive ? A.positive[e] != 0 : A.rating[e] >= A.pos_threshold;
  return pos && u >= 0 && u < A.n_users && it >= 0 && it < A.n_items;
}

// first[id] = the smallest index of a positive record that carries the id
// (0xFFFFFFFF from the memset: none). The plain read only skips atomics that
// cannot lower the value: it never rises.
__device__ __forceinline__ void split_note_first(unsigned *first, unsigned e) {
  if (*first > e) atomicMin(first, e);
}

__global__ __launch_bounds__(256) void split_first_kernel(bbgr_split_args A) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n) return;
  const int u = A.user[e], it = A.item[e];
  if (!split_positive(A, e, u, it)) return;
  split_note_first(reinterpret_cast<unsigned *>(A.user_map) + u, (unsigned)e);
  split_note_first(reinterpret_cast<unsigned *>(A.item_map) + it, (unsigned)e);
}

__device__ __forceinline__ bool split_flag(int code, int c) {
  if (c < 3) return (code & 3) == c + 1;
  return (code & (c == 3 ? CODE_FIRST_U : CODE_FIRST_I)) != 0;
}

// Per record its code, per tile the five flag counts.
__global__ __launch_bounds__(256) void split_code_kernel(bbgr_split_args A, uint8_t *code,
                                                         int *tile_counts) {
  __shared__ int s_cnt[4][SPLIT_NC];
  const long base = (long)blockIdx.x * SPLIT_TILE;
  const int t = threadIdx.x;
  int cnt[SPLIT_NC] = {0, 0, 0, 0, 0};   // wave-uniform
#pragma unroll
  for (int k = 0; k < SPLIT_ROUNDS; ++k) {
    const long e = base + k * 256 + t;
    int cd = 0;
    if (e < A.n) {
      const int u = A.user[e], it = A.item[e];
      if (split_positive(A, e, u, it)) {
        const unsigned long long h = A.hash32[e];
        cd = h < A.thr_train ? 1 : (h < A.thr_val ? 2 : 3);
        if ((unsigned)A.user_map[u] == (unsigned)e) cd |= CODE_FIRST_U;
        if ((unsigned)A.item_map[it] == (unsigned)e) cd |= CODE_FIRST_I;
      }
      code[e] = (uint8_t)cd;
    }
#pragma unroll
    for (int c = 0; c < SPLIT_NC; ++c) cnt[c] += __popcll(__ballot(split_flag(cd, c)));
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < SPLIT_NC; ++c) s_cnt[t >> 6][c] = cnt[c];
  }
  __syncthreads();
  if (t < SPLIT_NC)
    tile_counts[(long)blockIdx.x * SPLIT_NC + t] =
        (s_cnt[0][t] + s_cnt[1][t]) + (s_cnt[2][t] + s_cnt[3][t]);
}

// tile_counts[tile][c] -> the exclusive sum over the tiles before it, in place;
// totals (DEVICE int64 [5]) = {E_train, E_val, E_test, U', I'}. One workgroup,
// 1024 tiles a step (50M records: 24 steps).
__global__ __launch_bounds__(1024) void split_scan_kernel(long n_tiles, int *tile_counts,
                                                          long long *totals) {
  __shared__ int s_w[16][SPLIT_NC];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  int carry[SPLIT_NC] = {0, 0, 0, 0, 0};
  for (long base = 0; base < n_tiles; base += 1024) {
    const long i = base + t;
    int v[SPLIT_NC], x[SPLIT_NC];
#pragma unroll
    for (int c = 0; c < SPLIT_NC; ++c) {
      v[c] = i < n_tiles ? tile_counts[i * SPLIT_NC + c] : 0;
      x[c] = v[c];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x[c], o);
        if (l >= o) x[c] += y;
      }
      if (l == 63) s_w[w][c] = x[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SPLIT_NC; ++c) {
      int woff = 0, tot = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int ws = s_w[j][c];
        woff += j < w ? ws : 0;
        tot += ws;
      }
      if (i < n_tiles) tile_counts[i * SPLIT_NC + c] = carry[c] + woff + x[c] - v[c];
      carry[c] += tot;
    }
    __syncthreads();
  }
  if (t < SPLIT_NC) {
    // carry is the same in every thread; pick by a literal index
    long long total = carry[0];
    if (t == 1) total = carry[1];
    if (t == 2) total = carry[2];
    if (t == 3) total = carry[3];
    if (t == 4) total = carry[4];
    totals[t] = total;
  }
}

// The ranks of a tile's records under the flags C0 .. C0 + NC - 1, then the
// stores. EDGES: the three buckets -> the edge buffer; else the two "first"
// flags -> the id maps and their inverses.
template <bool EDGES>
__global__ __launch_bounds__(256) void split_scatter_kernel(bbgr_split_args A, const uint8_t *code,
                                                            const int *tile_off,
                                                            const long long *totals) {
  constexpr int C0 = EDGES ? 0 : 3, NC = EDGES ? 3 : 2;
  __shared__ int s_seg[SPLIT_SEGS][NC];
  const long base = (long)blockIdx.x * SPLIT_TILE;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const unsigned long long below = (1ull << l) - 1ull;
  int cd[SPLIT_ROUNDS];
#pragma unroll
  for (int k = 0; k < SPLIT_ROUNDS; ++k) {
    const long e = base + k * 256 + t;
    cd[k] = e < A.n ? code[e] : 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int tot = __popcll(__ballot(split_flag(cd[k], C0 + c)));
      if (l == 0) s_seg[k * 4 + w][c] = tot;
    }
  }
  __syncthreads();
  if (t < NC) {   // exclusive over the tile's 32 runs, from the tile's own offset
    int run = tile_off[(long)blockIdx.x * SPLIT_NC + C0 + t];
    for (int j = 0; j < SPLIT_SEGS; ++j) {
      const int v = s_seg[j][t];
      s_seg[j][t] = run;
      run += v;
    }
  }
  __syncthreads();
  long bucket_base[3] = {0, 0, 0};
  if (EDGES) {
    bucket_base[1] = (long)totals[0];
    bucket_base[2] = (long)(totals[0] + totals[1]);
  }
#pragma unroll
  for (int k = 0; k < SPLIT_ROUNDS; ++k) {
    const long e = base + k * 256 + t;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool f = split_flag(cd[k], C0 + c);
      const long rank = s_seg[k * 4 + w][c] + __popcll(__ballot(f) & below);
      if (!f) continue;
      if (EDGES) {
        const long dst = bucket_base[c] + rank;
        if (dst < A.ld_edges) {   // always: at most n positives, ld_edges >= n
          A.edges[dst] = A.user_map[A.user[e]];
          A.edges[A.ld_edges + dst] = A.item_map[A.item[e]];
        }
      } else if (c == 0) {
        const int u = A.user[e];
        if (rank < A.n_users) {   // always: one first record per id
          A.user_src[rank] = u;
          A.user_map[u] = (int)rank;
        }
      } else {
        const int it = A.item[e];
        if (rank < A.n_items) {
          A.item_src[rank] = it;
          A.item_map[it] = (int)rank;
        }
      }
    }
  }
}

static long split_tiles(long n) { return (n + SPLIT_TILE - 1) / SPLIT_TILE; }

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_md5_pair_hash(int64_t n, const int32_t *user, const int32_t *item,
                                  const uint8_t *user_data, const int64_t *user_offsets,
                                  int32_t n_users, const uint8_t *item_data,
                                  const int64_t *item_offsets, int32_t n_items,
                                  const uint8_t *keep, uint32_t *hash32, bbgr_stream_t stream) {
  static const char *fn = "bbgr_md5_pair_hash";
  BBGR_REQUIRE_IN(fn, n >= 0 && n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, n_users >= 0 && n_users < INT_MAX, "n_users out of range");
  BBGR_REQUIRE_IN(fn, n_items >= 0 && n_items < INT_MAX, "n_items out of range");
  if (n == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, n_users > 0 && n_items > 0, "records but no n_users / n_items");
  BBGR_REQUIRE_IN(fn, user, "null user");
  BBGR_REQUIRE_IN(fn, item, "null item");
  BBGR_REQUIRE_IN(fn, user_data, "null user_data");
  BBGR_REQUIRE_IN(fn, user_offsets, "null user_offsets");
  BBGR_REQUIRE_IN(fn, item_data, "null item_data");
  BBGR_REQUIRE_IN(fn, item_offsets, "null item_offsets");
  BBGR_REQUIRE_IN(fn, hash32, "null hash32");
  Md5Params P;
  P.n = (long)n;
  P.user = user;
  P.item = item;
  P.user_data = user_data;
  P.user_offsets = reinterpret_cast<const long long *>(user_offsets);
  P.n_users = n_users;
  P.item_data = item_data;
  P.item_offsets = reinterpret_cast<const long long *>(item_offsets);
  P.n_items = n_items;
  P.keep = keep;
  P.hash32 = hash32;
  hipLaunchKernelGGL(md5_pair_hash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), P);
  BBGR_LAUNCHED("md5_pair_hash_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_split_edges(const bbgr_split_args *a, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_split_edges";
  BBGR_REQUIRE_IN(fn, a, "null args");
  BBGR_REQUIRE_IN(fn, a->n >= 0 && a->n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, a->n_users >= 0 && a->n_users < INT_MAX, "n_users out of range");
  BBGR_REQUIRE_IN(fn, a->n_items >= 0 && a->n_items < INT_MAX, "n_items out of range");
  BBGR_REQUIRE_IN(fn, a->thr_val <= SPLIT_THR_MAX, "thr_val > 2^32");
  BBGR_REQUIRE_IN(fn, a->thr_train <= a->thr_val, "thr_train > thr_val");
  if (a->n > 0) {
    BBGR_REQUIRE_IN(fn, a->n_users > 0 && a->n_items > 0, "records but no n_users / n_items");
    BBGR_REQUIRE_IN(fn, a->user, "null user");
    BBGR_REQUIRE_IN(fn, a->item, "null item");
    BBGR_REQUIRE_IN(fn, a->positive || a->rating, "null positive and null rating");
    BBGR_REQUIRE_IN(fn, a->hash32, "null hash32");
    BBGR_REQUIRE_IN(fn, a->user_map, "null user_map");
    BBGR_REQUIRE_IN(fn, a->item_map, "null item_map");
    BBGR_REQUIRE_IN(fn, a->user_src, "null user_src");
    BBGR_REQUIRE_IN(fn, a->item_src, "null item_src");
    BBGR_REQUIRE_IN(fn, a->edges, "null edges");
    BBGR_REQUIRE_IN(fn, a->ld_edges >= a->n, "ld_edges < n");
    BBGR_REQUIRE_IN(fn, a->counts, "null counts");
  }
  const long n = (long)a->n, n_tiles = split_tiles(n);
  // one code byte per record, then SPLIT_NC counts per tile (and one tile more)
  Carver C;
  const size_t off_code = C.take((size_t)n);
  const size_t off_tiles = C.take_n<int>(SPLIT_NC * (size_t)(n_tiles + 1));
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query || n == 0) return rc;
  hipStream_t st = as_stream(stream);
  uint8_t *code = ws_at<uint8_t>(workspace, off_code);
  int *tiles = ws_at<int>(workspace, off_tiles);
  long long *totals = reinterpret_cast<long long *>(a->counts);
  BBGR_HIP(hipMemsetAsync(a->user_map, 0xff, sizeof(int) * (size_t)a->n_users, st));
  BBGR_HIP(hipMemsetAsync(a->item_map, 0xff, sizeof(int) * (size_t)a->n_items, st));
  hipLaunchKernelGGL(split_first_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *a);
  BBGR_LAUNCHED("split_first_kernel");
  hipLaunchKernelGGL(split_code_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, *a, code,
                     tiles);
  BBGR_LAUNCHED("split_code_kernel");
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(1024), 0, st, n_tiles, tiles, totals);
  BBGR_LAUNCHED("split_scan_kernel");
  hipLaunchKernelGGL(split_scatter_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, st, *a,
                     (const uint8_t *)code, (const int *)tiles, (const long long *)totals);
  BBGR_LAUNCHED("split_scatter_kernel<ids>");
  hipLaunchKernelGGL(split_scatter_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, st, *a,
                     (const uint8_t *)code, (const int *)tiles, (const long long *)totals);
  BBGR_LAUNCHED("split_scatter_kernel<edges>");
  return BBGR_OK;
}
