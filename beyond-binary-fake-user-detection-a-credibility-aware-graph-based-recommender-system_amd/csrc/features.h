// What the two feature translation units share (features.hip,
// features_v2.hip).
//
// The row pass. Every pass that walks a CSR row is a small struct (a Pass)
// handed by value to the two kernels below: feat_rows_kernel gives every row to
// one lane, which either runs P.short_row(r) or, for a row of more than
// Pass::LONG_ROW records, appends it to a list through an integer atomic
// counter (the list's order reaches no result); feat_rows_long_kernel strides
// FEAT_LONG_GRID workgroups over that list and runs P.long_row(r) with all 256
// threads. feat_row_pass is the one host block: the carve of the list, the
// reset of the counter, the two launches.
//
// SumPass is the second layer for the passes that only add things up: the
// pass says what a record adds (accumulate), how its accumulator is summed
// over a workgroup (Acc::block_sum) and what a row stores (store); the short
// row is then one lane adding in row order from a zero accumulator, the long
// row thread t adding slots t, t + 256, ... and feat_block_sum's fixed shape:
// a xor tree over a wave, then ((w0 + w1) + w2) + w3. The shape depends on the
// row's length alone, so two runs give the same bits.
//
// The user pass of both feature sets: UserCounts (the integer part of the
// accumulator), feat_user_head (counts, label, columns 0 to 2) and the packed
// record of feat_pack_kernel. Then the rounded rating, an entropy term and the
// host check of the columns.
#pragma once

#include "common.h"

#include <limits.h>
#include <math.h>

namespace bbgr {

constexpr int FEAT_LONG_ROW = 512;          // records; above: one workgroup per row
constexpr int FEAT_LONG_GRID = 256;         // workgroups striding over the long-row list

// clamp(round_half_even(rating), 1, 5): Python's round() is half-to-even, as
// rintf is in the default rounding mode. The clamp runs in float so that no
// out-of-range value is converted; a NaN gives 1.
__device__ __forceinline__ int feat_ri(float rating) {
  return (int)fminf(fmaxf(rintf(rating), 1.f), 5.f);
}

__device__ __forceinline__ bool feat_has_ts(const bbgr_feat_columns &C, long e) {
  return C.ts_valid == nullptr || C.ts_valid[e] != 0;
}

// Sum over the 256 threads of a workgroup in a fixed order; every thread
// returns the total. s: 4 entries of LDS, free again on return.
template <typename T> __device__ __forceinline__ T feat_block_sum(T v, T *s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = ((s[0] + s[1]) + s[2]) + s[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double feat_plogp(double H, int c, double n) {
#pragma clang fp contract(off)
  if (c > 0) {
    const double p = (double)c / n;
    const double t = p * log(p);
    H -= t;
  }
  return H;
}

// ---------------------------------------------------------------------------
// The row pass
// ---------------------------------------------------------------------------
struct LongRows {
  int *count;   // zeroed before the short-row launch
  int *rows;
  int cap;
};

template <class Pass>
__global__ __launch_bounds__(256) void feat_rows_kernel(Pass P, int n_rows, LongRows L) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  if (P.length(r) > Pass::LONG_ROW) {
    const int pos = atomicAdd(L.count, 1);
    if (pos < L.cap) L.rows[pos] = r;   // always: fewer than n / LONG_ROW such rows
    return;
  }
  P.short_row(r);
}

template <class Pass>
__global__ __launch_bounds__(256) void feat_rows_long_kernel(Pass P, LongRows L) {
  const int n_long = min(*L.count, L.cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) P.long_row(L.rows[j]);
}

// The list's bytes at the head of a pass's workspace: the counter, then at
// +256 the rows. A long row has more than `row` records, so there are fewer
// than n / row of them.
inline size_t feat_long_bytes(long n, int row = FEAT_LONG_ROW) {
  return align_up(256 + sizeof(int) * (size_t)(n / row + 1));
}

// One pass over n_rows rows of n records in all. The long-row kernel is
// launched only when a row can be long.
template <class Pass>
int feat_row_pass(const char *fn, const Pass &P, int n_rows, long n, void *workspace,
                  hipStream_t st) {
  const LongRows L{static_cast<int *>(workspace),
                   reinterpret_cast<int *>(static_cast<char *>(workspace) + 256),
                   (int)(n / Pass::LONG_ROW + 1)};
  BBGR_HIP(hipMemsetAsync(L.count, 0, sizeof(int), st));
  hipLaunchKernelGGL(feat_rows_kernel<Pass>, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                     st, P, n_rows, L);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && n > Pass::LONG_ROW) {
    hipLaunchKernelGGL(feat_rows_long_kernel<Pass>, dim3(FEAT_LONG_GRID), dim3(256), 0, st, P, L);
    e = hipGetLastError();
  }
  return e == hipSuccess ? BBGR_OK : hip_fail(e, (std::string(fn) + ": launch of a row kernel").c_str());
}

// A pass that sums over its rows (rows r of indptr). Derived has Acc (zero
// when default-constructed, with block_sum()), accumulate(r, start, step, acc)
// over the row's slots start, start + step, .. and store(r, n, acc).
template <class Derived> struct SumPass {
  static constexpr int LONG_ROW = FEAT_LONG_ROW;
  const int *indptr;
  __device__ __forceinline__ int length(int r) const { return indptr[r + 1] - indptr[r]; }
  __device__ __forceinline__ void short_row(int r) const {
    const Derived &D = static_cast<const Derived &>(*this);
    const int n = length(r);
    typename Derived::Acc a;
    D.accumulate(r, 0, 1, a);
    D.store(r, n, a);
  }
  __device__ __forceinline__ void long_row(int r) const {
    const Derived &D = static_cast<const Derived &>(*this);
    const int n = length(r);   // read before the barriers, which would have it read again
    typename Derived::Acc a;
    D.accumulate(r, threadIdx.x, 256, a);
    a.block_sum();
    if (threadIdx.x == 0) D.store(r, n, a);
  }
};

// ---------------------------------------------------------------------------
// The user pass of both feature sets
// ---------------------------------------------------------------------------
// What the pass needs of a record, in one 16-byte word: gathered by record id,
// separate columns cost a memory line each per record, this one. x: item,
// y: n_tokens, z: the raw rating's bits (RAW_RATING) or n_unique_tokens,
// w: ri | 8 when helpful_vote > 5.
template <bool RAW_RATING>
__global__ __launch_bounds__(256) void feat_pack_kernel(bbgr_feat_columns C, int4 *packed) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= C.n) return;
  const float r = C.rating[e];
  packed[e] = make_int4(C.item[e], C.n_tokens[e],
                        RAW_RATING ? __float_as_int(r) : C.n_unique_tokens[e],
                        feat_ri(r) | (C.helpful_vote[e] > 5 ? 8 : 0));
}

template <bool RAW_RATING>
int feat_pack(const bbgr_feat_columns *c, int4 *packed, hipStream_t st) {
  if (c->n == 0) return BBGR_OK;
  hipLaunchKernelGGL(feat_pack_kernel<RAW_RATING>, dim3((unsigned)((c->n + 255) / 256)), dim3(256),
                     0, st, *c, packed);
  BBGR_LAUNCHED("feat_pack_kernel");
  return BBGR_OK;
}

// The integer part of a user's accumulator; each feature set adds its doubles.
struct UserCounts {
  int helpful = 0;
  int h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0;   // histogram of the rounded rating
  int distinct = 0;                             // distinct day buckets
  int n_ts = 0;                                 // records with a timestamp: not summed, the row's
  // w: the packed word's ri | 8 * helpful
  __device__ __forceinline__ void add(int w) {
    const int ri = w & 7;
    h1 += ri == 1;
    h2 += ri == 2;
    h3 += ri == 3;
    h4 += ri == 4;
    h5 += ri == 5;
    helpful += w >> 3;
  }
  // The row's sorted buckets: a slot counts when it differs from the one before.
  __device__ __forceinline__ void add_buckets(const int *b_indptr, const int *b_bucket, int u,
                                              int start, int step) {
    const int bb = b_indptr[u], be = b_indptr[u + 1];
    n_ts = be - bb;
    for (int p = bb + start; p < be; p += step)
      distinct += (p == bb || b_bucket[p] != b_bucket[p - 1]) ? 1 : 0;
  }
  __device__ __forceinline__ void block_sum() {
    __shared__ int s_i[4];
    helpful = feat_block_sum(helpful, s_i);
    h1 = feat_block_sum(h1, s_i);
    h2 = feat_block_sum(h2, s_i);
    h3 = feat_block_sum(h3, s_i);
    h4 = feat_block_sum(h4, s_i);
    h5 = feat_block_sum(h5, s_i);
    distinct = feat_block_sum(distinct, s_i);
  }
};

// What both feature sets store of a user alike (A: either args struct): the
// two counts, the Ru label, columns 0 to 2. False for a user with no record,
// whose seven columns are NaN and who is unlabeled (the graph pass's row).
template <class Args>
__device__ __forceinline__ bool feat_user_head(const Args &A, int u, int n, const UserCounts &a) {
#pragma clang fp contract(off)
  float *x = A.user_x + 7L * u;
  A.total_reviews[u] = n;
  A.helpful_reviews[u] = a.helpful;
  if (n == 0) {
#pragma unroll
    for (int f = 0; f < 7; ++f) x[f] = NAN;
    A.user_y[u] = -1;
    return false;
  }
  const double dn = (double)n;
  const double Ru = (double)a.helpful / dn;
  A.user_y[u] = Ru >= 0.7 ? 1 : (Ru <= 0.3 ? 0 : -1);
  double H = 0.0;
  H = feat_plogp(H, a.h1, dn);
  H = feat_plogp(H, a.h2, dn);
  H = feat_plogp(H, a.h3, dn);
  H = feat_plogp(H, a.h4, dn);
  H = feat_plogp(H, a.h5, dn);
  x[0] = (float)Ru;
  x[1] = (float)H;
  x[2] = (float)((double)(a.h1 + a.h5) / dn);
  return true;
}

inline int feat_columns_ok(const char *fn, const bbgr_feat_columns *c) {
  BBGR_REQUIRE_IN(fn, c, "null columns");
  BBGR_REQUIRE_IN(fn, c->n >= 0 && c->n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, c->n_users >= 0 && c->n_users < INT_MAX, "n_users out of range");
  BBGR_REQUIRE_IN(fn, c->n_items >= 0, "n_items < 0");
  if (c->n == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, c->n_users > 0 && c->n_items > 0, "records but no n_users / n_items");
  BBGR_REQUIRE_IN(fn, c->user, "null user");
  BBGR_REQUIRE_IN(fn, c->item, "null item");
  BBGR_REQUIRE_IN(fn, c->rating, "null rating");
  BBGR_REQUIRE_IN(fn, c->helpful_vote, "null helpful_vote");
  BBGR_REQUIRE_IN(fn, c->verified, "null verified");
  BBGR_REQUIRE_IN(fn, c->timestamp, "null timestamp");
  BBGR_REQUIRE_IN(fn, c->n_tokens, "null n_tokens");
  BBGR_REQUIRE_IN(fn, c->n_unique_tokens, "null n_unique_tokens");
  return BBGR_OK;
}

}  // namespace bbgr
