// Ru labels, user features, item features and edge attributes from numeric
// per-review columns (main.py:153-196, :247-373, :423-570): what the loaded
// credibility graph (SlasGraph) is made of.
//
// A record is one review with a user, an item and a rating; the columns hold
// one entry per record in file order. Records are grouped by the
// reference-order CSR (a stable bbgr_csr_build keyed by the id alone, its
// permutation as the record ids: a row lists its records in file order), once
// by user and once by item; a third
// build over (user, day bucket) of the records that have a timestamp gives
// each user's buckets sorted, so the distinct-bucket count is a boundary count.
//
// Every sum is taken in double in a fixed order and without float atomics:
// a row of at most FEAT_LONG_ROW records is summed by one lane in file order
// (the order of the reference's loops), a longer row by one workgroup: thread
// t takes the records t, t + 256, ... in order, a xor tree adds the lanes of a
// wave and the four waves are added in wave order. The shape depends on the
// row's length alone, so two runs give the same bits. The long rows are handed
// from the short-row kernel to the long-row kernel through a list filled with
// an integer atomic counter; the list's order does not reach any result.
// Results are rounded to float once, at the store.
//
// Measured at 1M and 50M records in DESIGN 4d (tools/features_bench.py).
#include "common.h"
#include "features.h"

#include <limits.h>
#include <math.h>

namespace bbgr {

constexpr long long FEAT_TAU_MS = 86400000LL;   // one-day buckets (TAU_MS)

__host__ __device__ __forceinline__ long long feat_floor_div(long long a, long long b) {
  long long q = a / b;
  if (a % b < 0) --q;   // b > 0: Python's //
  return q;
}

// ---------------------------------------------------------------------------
// Global statistics: stats[0..3] = min and max timestamp and the count of the
// records that have one, and the sum of n_tokens. Integers: the atomics below
// commute exactly.
// ---------------------------------------------------------------------------
__global__ void feat_stats_init_kernel(long long *stats) {
  stats[0] = LLONG_MAX;
  stats[1] = LLONG_MIN;
  stats[2] = 0;
  stats[3] = 0;
}

__global__ __launch_bounds__(256) void feat_stats_kernel(bbgr_feat_columns C, long long *stats) {
  long long lo = LLONG_MAX, hi = LLONG_MIN, cnt = 0, len = 0;
  const long step = (long)gridDim.x * 256;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < C.n; e += step) {
    len += C.n_tokens[e];
    if (feat_has_ts(C, e)) {
      const long long t = C.timestamp[e];
      lo = t < lo ? t : lo;
      hi = t > hi ? t : hi;
      ++cnt;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
    cnt += __shfl_xor(cnt, o);
    len += __shfl_xor(len, o);
  }
  // the four waves meet in LDS: one set of atomics per workgroup, so that the
  // four shared addresses see a few thousand atomics however long the columns
  __shared__ long long s_part[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_part[w][0] = lo;
    s_part[w][1] = hi;
    s_part[w][2] = cnt;
    s_part[w][3] = len;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 4; ++j) {
      lo = s_part[j][0] < lo ? s_part[j][0] : lo;
      hi = s_part[j][1] > hi ? s_part[j][1] : hi;
      cnt += s_part[j][2];
      len += s_part[j][3];
    }
    if (cnt) {
      atomicMin(&stats[0], lo);
      atomicMax(&stats[1], hi);
      atomicAdd(reinterpret_cast<unsigned long long *>(&stats[2]), (unsigned long long)cnt);
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(&stats[3]), (unsigned long long)len);
  }
}

// ---------------------------------------------------------------------------
// (row, column) of the bucket CSR: a record with a timestamp goes to its
// user's row with its day bucket less the smallest bucket, one without to the
// spare row n_users, which nothing reads.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_buckets_kernel(bbgr_feat_columns C, long long bucket_min,
                                                           int *rows, int *cols) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= C.n) return;
  const int u = C.user[e];
  const bool ok = feat_has_ts(C, e) && u >= 0 && u < C.n_users;
  rows[e] = ok ? u : C.n_users;
  cols[e] = ok ? (int)(feat_floor_div(C.timestamp[e], FEAT_TAU_MS) - bucket_min) : 0;
}

// ---------------------------------------------------------------------------
// Per-item statistics: the count, the sum of the raw rating (item_x's mean)
// and the sum of the rounded rating (the mean the user deviation is taken from)
// ---------------------------------------------------------------------------
struct ItemAcc {
  double sum_r = 0.0;
  long long sum_ri = 0;
};

__device__ __forceinline__ void feat_item_acc(const bbgr_feat_columns &C, const int *eid, int rb,
                                              int re, int start, int step, ItemAcc &a) {
#pragma clang fp contract(off)
#pragma unroll 4
  for (int p = rb + start; p < re; p += step) {
    const float r = C.rating[eid[p]];
    a.sum_r += (double)r;
    a.sum_ri += feat_ri(r);
  }
}

__device__ __forceinline__ void feat_item_store(int i, int n, const ItemAcc &a, float *item_x,
                                                double *item_rbar) {
  const double den = n > 0 ? (double)n : 1.0;
  item_x[2L * i] = (float)(a.sum_r / den);
  item_x[2L * i + 1] = (float)n;
  item_rbar[i] = (double)a.sum_ri / den;
}

__global__ __launch_bounds__(256) void feat_items_kernel(bbgr_feat_columns C, const int *indptr,
                                                         const int *eid, float *item_x,
                                                         double *item_rbar, int *long_count,
                                                         int *long_rows, int long_cap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C.n_items) return;
  const int rb = indptr[i], re = indptr[i + 1];
  if (re - rb > FEAT_LONG_ROW) {
    const int pos = atomicAdd(long_count, 1);
    if (pos < long_cap) long_rows[pos] = i;   // always, for an indptr that ends at n
    return;
  }
  ItemAcc a;
  feat_item_acc(C, eid, rb, re, 0, 1, a);
  feat_item_store(i, re - rb, a, item_x, item_rbar);
}

__global__ __launch_bounds__(256) void feat_items_long_kernel(bbgr_feat_columns C,
                                                              const int *indptr, const int *eid,
                                                              float *item_x, double *item_rbar,
                                                              const int *long_count,
                                                              const int *long_rows, int long_cap) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int n_long = min(*long_count, long_cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int i = long_rows[j];
    const int rb = indptr[i], re = indptr[i + 1];
    ItemAcc a;
    feat_item_acc(C, eid, rb, re, threadIdx.x, 256, a);
    a.sum_r = feat_block_sum(a.sum_r, s_d);
    a.sum_ri = feat_block_sum(a.sum_ri, s_l);
    if (threadIdx.x == 0) feat_item_store(i, re - rb, a, item_x, item_rbar);
  }
}

// ---------------------------------------------------------------------------
// Per-user label and features
// ---------------------------------------------------------------------------
struct UserAcc {
  int helpful = 0;
  int h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0;   // histogram of the rounded rating
  int distinct = 0;                             // distinct day buckets
  double aad = 0.0, ld = 0.0, rd = 0.0;
};

// What the user pass needs of a record, in one 16-byte word: gathered by
// record id, five separate columns cost five memory lines per record, this one.
// x: item, y: n_tokens, z: n_unique_tokens, w: ri | 8 when helpful_vote > 5.
__global__ __launch_bounds__(256) void feat_pack_kernel(bbgr_feat_columns C, int4 *packed) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= C.n) return;
  packed[e] = make_int4(C.item[e], C.n_tokens[e], C.n_unique_tokens[e],
                        feat_ri(C.rating[e]) | (C.helpful_vote[e] > 5 ? 8 : 0));
}

__device__ __forceinline__ void feat_user_acc(const bbgr_feat_columns &C,
                                              const bbgr_feat_user_args &A, const int4 *packed,
                                              int rb, int re, int bb, int be, int start, int step,
                                              UserAcc &a) {
#pragma clang fp contract(off)
#pragma unroll 4
  for (int p = rb + start; p < re; p += step) {
    const int4 r = packed[A.u_eid[p]];
    const int ri = r.w & 7;
    a.h1 += ri == 1;
    a.h2 += ri == 2;
    a.h3 += ri == 3;
    a.h4 += ri == 4;
    a.h5 += ri == 5;
    a.helpful += r.w >> 3;
    const double rbar = r.x >= 0 && r.x < C.n_items ? A.item_rbar[r.x] : (double)NAN;
    a.aad += fabs((double)ri - rbar);
    const int L = r.y;
    if (L > 0) a.ld += (double)r.z / (double)L;
    a.rd += fabs((double)L - A.global_avg_len);
  }
  for (int p = bb + start; p < be; p += step)
    a.distinct += (p == bb || A.b_bucket[p] != A.b_bucket[p - 1]) ? 1 : 0;
}

__device__ __forceinline__ void feat_user_store(const bbgr_feat_user_args &A, int u, int n,
                                                int n_ts, const UserAcc &a) {
#pragma clang fp contract(off)
  float *x = A.user_x + 7L * u;
  A.total_reviews[u] = n;
  A.helpful_reviews[u] = a.helpful;
  if (n == 0) {   // no record: the NaN row of the graph pass, unlabeled
#pragma unroll
    for (int f = 0; f < 7; ++f) x[f] = NAN;
    A.user_y[u] = -1;
    return;
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
  x[3] = (float)(a.aad / dn);
  x[4] = (float)(n_ts - a.distinct);   // sum over the buckets of (count - 1)
  x[5] = (float)(a.ld / dn);
  x[6] = (float)(a.rd / dn);
}

__global__ __launch_bounds__(256) void feat_users_kernel(bbgr_feat_columns C, bbgr_feat_user_args A,
                                                         const int4 *packed, int *long_count,
                                                         int *long_rows,
                                                         int long_cap) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= C.n_users) return;
  const int rb = A.u_indptr[u], re = A.u_indptr[u + 1];
  if (re - rb > FEAT_LONG_ROW) {
    const int pos = atomicAdd(long_count, 1);
    if (pos < long_cap) long_rows[pos] = u;   // always, for an indptr that ends at n
    return;
  }
  const int bb = A.b_indptr[u], be = A.b_indptr[u + 1];
  UserAcc a;
  feat_user_acc(C, A, packed, rb, re, bb, be, 0, 1, a);
  feat_user_store(A, u, re - rb, be - bb, a);
}

__global__ __launch_bounds__(256) void feat_users_long_kernel(bbgr_feat_columns C,
                                                              bbgr_feat_user_args A,
                                                              const int4 *packed,
                                                              const int *long_count,
                                                              const int *long_rows, int long_cap) {
  __shared__ double s_d[4];
  __shared__ int s_i[4];
  const int n_long = min(*long_count, long_cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int u = long_rows[j];
    const int rb = A.u_indptr[u], re = A.u_indptr[u + 1];
    const int bb = A.b_indptr[u], be = A.b_indptr[u + 1];
    UserAcc a;
    feat_user_acc(C, A, packed, rb, re, bb, be, threadIdx.x, 256, a);
    a.helpful = feat_block_sum(a.helpful, s_i);
    a.h1 = feat_block_sum(a.h1, s_i);
    a.h2 = feat_block_sum(a.h2, s_i);
    a.h3 = feat_block_sum(a.h3, s_i);
    a.h4 = feat_block_sum(a.h4, s_i);
    a.h5 = feat_block_sum(a.h5, s_i);
    a.distinct = feat_block_sum(a.distinct, s_i);
    a.aad = feat_block_sum(a.aad, s_d);
    a.ld = feat_block_sum(a.ld, s_d);
    a.rd = feat_block_sum(a.rd, s_d);
    if (threadIdx.x == 0) feat_user_store(A, u, re - rb, be - bb, a);
  }
}

// ---------------------------------------------------------------------------
// Per-edge attributes, EDGE_ATTR_KEYS order: verified, rating_align, rating,
// timestamp_norm, helpful_vote. One record per thread, a streaming pass. The
// five floats of a record are 20 bytes apart from the next record's, so a
// workgroup's 256 rows (5120 bytes, 16-byte aligned for a 16-byte aligned
// table) meet in LDS and leave as 320 whole 16-byte stores.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_edges_kernel(bbgr_feat_columns C, const float *item_x,
                                                         long long ts_min, long long ts_max,
                                                         float *edge_attr) {
#pragma clang fp contract(off)
  __shared__ float4 s_rows[320];
  float *s = reinterpret_cast<float *>(s_rows);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < C.n) {
    const float r = C.rating[e];
    const int it = C.item[e];
    const float mean = it >= 0 && it < C.n_items ? item_x[2L * it] : NAN;
    float tsn = NAN;
    if (ts_max > ts_min && feat_has_ts(C, e))
      tsn = (float)((double)(C.timestamp[e] - ts_min) / (double)(ts_max - ts_min));
    float *o = s + 5 * threadIdx.x;   // stride 5 words: no bank conflict
    o[0] = C.verified[e] ? 1.f : 0.f;
    o[1] = (float)(1.0 - fabs((double)r - (double)mean) / 4.0);
    o[2] = r;
    o[3] = tsn;
    o[4] = (float)C.helpful_vote[e];
  }
  __syncthreads();
  const long base = (long)blockIdx.x * 1280;   // floats before this workgroup's rows
  const long total = 5 * C.n;
  for (int q = threadIdx.x; q < 320; q += 256) {
    const long off = base + 4L * q;
    if (off + 4 <= total) {
      *reinterpret_cast<float4 *>(edge_attr + off) = s_rows[q];
    } else {
      for (int k = 0; k < 4; ++k)
        if (off + k < total) edge_attr[off + k] = s[4 * q + k];
    }
  }
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_feat_stats(const bbgr_feat_columns *c, int64_t *stats, bbgr_stream_t stream) {
  int rc = feat_columns_ok("bbgr_feat_stats", c);
  if (rc) return rc;
  BBGR_REQUIRE(stats, "bbgr_feat_stats: null stats");
  hipStream_t st = as_stream(stream);
  long long *s = reinterpret_cast<long long *>(stats);
  hipLaunchKernelGGL(feat_stats_init_kernel, dim3(1), dim3(1), 0, st, s);
  BBGR_LAUNCHED("feat_stats_init_kernel");
  if (c->n == 0) return BBGR_OK;
  const long blocks = (c->n + 255) / 256;
  hipLaunchKernelGGL(feat_stats_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256),
                     0, st, *c, s);
  BBGR_LAUNCHED("feat_stats_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_feat_buckets(const bbgr_feat_columns *c, int64_t ts_min, int64_t ts_max,
                                 int32_t *rows, int32_t *cols, int32_t *n_cols,
                                 bbgr_stream_t stream) {
  int rc = feat_columns_ok("bbgr_feat_buckets", c);
  if (rc) return rc;
  BBGR_REQUIRE(n_cols, "bbgr_feat_buckets: null n_cols");
  long long bmin = 0, width = 1;
  if (ts_min <= ts_max) {   // some record has a timestamp
    bmin = feat_floor_div(ts_min, FEAT_TAU_MS);
    // at most 2^64 / 86400000 < 2^38 buckets apart: no overflow
    width = feat_floor_div(ts_max, FEAT_TAU_MS) - bmin + 1;
    if (width > INT_MAX) {
      set_error("bbgr_feat_buckets: timestamp: the day buckets of ts_min and ts_max are %lld "
                "apart; the bucket range must fit int32", width - 1);
      return BBGR_ERR_INVALID;
    }
  }
  *n_cols = (int32_t)width;
  if (c->n == 0) return BBGR_OK;
  BBGR_REQUIRE(rows, "bbgr_feat_buckets: null rows");
  BBGR_REQUIRE(cols, "bbgr_feat_buckets: null cols");
  hipLaunchKernelGGL(feat_buckets_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), *c, bmin, rows, cols);
  BBGR_LAUNCHED("feat_buckets_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_feat_items(const bbgr_feat_columns *c, const int32_t *i_indptr,
                               const int32_t *i_eid, float *item_x, double *item_rbar,
                               void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  int rc = feat_columns_ok("bbgr_feat_items", c);
  if (rc) return rc;
  BBGR_REQUIRE(workspace_bytes, "bbgr_feat_items: null workspace_bytes");
  bool query;
  rc = feat_workspace("bbgr_feat_items", feat_long_bytes((long)c->n), workspace, workspace_bytes,
                      &query);
  if (rc || query) return rc;
  if (c->n_items == 0) return BBGR_OK;
  BBGR_REQUIRE(i_indptr, "bbgr_feat_items: null i_indptr");
  BBGR_REQUIRE(c->n == 0 || i_eid, "bbgr_feat_items: null i_eid");
  BBGR_REQUIRE(item_x, "bbgr_feat_items: null item_x");
  BBGR_REQUIRE(item_rbar, "bbgr_feat_items: null item_rbar");
  hipStream_t st = as_stream(stream);
  int *long_count = static_cast<int *>(workspace);
  int *long_rows = reinterpret_cast<int *>(static_cast<char *>(workspace) + 256);
  const int long_cap = (int)(c->n / FEAT_LONG_ROW + 1);
  BBGR_HIP(hipMemsetAsync(long_count, 0, sizeof(int), st));
  hipLaunchKernelGGL(feat_items_kernel, dim3((unsigned)((c->n_items + 255) / 256)), dim3(256), 0,
                     st, *c, i_indptr, i_eid, item_x, item_rbar, long_count, long_rows, long_cap);
  BBGR_LAUNCHED("feat_items_kernel");
  if (c->n > FEAT_LONG_ROW) {
    hipLaunchKernelGGL(feat_items_long_kernel, dim3(FEAT_LONG_GRID), dim3(256), 0, st, *c,
                       i_indptr, i_eid, item_x, item_rbar, long_count, long_rows, long_cap);
    BBGR_LAUNCHED("feat_items_long_kernel");
  }
  return BBGR_OK;
}

extern "C" int bbgr_feat_users(const bbgr_feat_columns *c, const bbgr_feat_user_args *a,
                               void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  int rc = feat_columns_ok("bbgr_feat_users", c);
  if (rc) return rc;
  BBGR_REQUIRE(a, "bbgr_feat_users: null args");
  BBGR_REQUIRE(workspace_bytes, "bbgr_feat_users: null workspace_bytes");
  bool query;
  // the long-row list, then the packed records
  const size_t off_packed = feat_long_bytes((long)c->n);
  rc = feat_workspace("bbgr_feat_users", off_packed + align_up(sizeof(int4) * (size_t)c->n),
                      workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_users == 0) return BBGR_OK;
  BBGR_REQUIRE(a->u_indptr, "bbgr_feat_users: null u_indptr");
  BBGR_REQUIRE(a->b_indptr, "bbgr_feat_users: null b_indptr");
  if (c->n > 0) {
    BBGR_REQUIRE(a->u_eid, "bbgr_feat_users: null u_eid");
    BBGR_REQUIRE(a->b_bucket, "bbgr_feat_users: null b_bucket");
    BBGR_REQUIRE(a->item_rbar, "bbgr_feat_users: null item_rbar");
  }
  BBGR_REQUIRE(a->user_x, "bbgr_feat_users: null user_x");
  BBGR_REQUIRE(a->user_y, "bbgr_feat_users: null user_y");
  BBGR_REQUIRE(a->total_reviews, "bbgr_feat_users: null total_reviews");
  BBGR_REQUIRE(a->helpful_reviews, "bbgr_feat_users: null helpful_reviews");
  hipStream_t st = as_stream(stream);
  int *long_count = static_cast<int *>(workspace);
  int *long_rows = reinterpret_cast<int *>(static_cast<char *>(workspace) + 256);
  const int long_cap = (int)(c->n / FEAT_LONG_ROW + 1);
  BBGR_HIP(hipMemsetAsync(long_count, 0, sizeof(int), st));
  int4 *packed = reinterpret_cast<int4 *>(static_cast<char *>(workspace) + off_packed);
  if (c->n > 0) {
    hipLaunchKernelGGL(feat_pack_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, st,
                       *c, packed);
    BBGR_LAUNCHED("feat_pack_kernel");
  }
  hipLaunchKernelGGL(feat_users_kernel, dim3((unsigned)((c->n_users + 255) / 256)), dim3(256), 0,
                     st, *c, *a, packed, long_count, long_rows, long_cap);
  BBGR_LAUNCHED("feat_users_kernel");
  if (c->n > FEAT_LONG_ROW) {
    hipLaunchKernelGGL(feat_users_long_kernel, dim3(FEAT_LONG_GRID), dim3(256), 0, st, *c, *a,
                       packed, long_count, long_rows, long_cap);
    BBGR_LAUNCHED("feat_users_long_kernel");
  }
  return BBGR_OK;
}

extern "C" int bbgr_feat_edges(const bbgr_feat_columns *c, const float *item_x, int64_t ts_min,
                               int64_t ts_max, float *edge_attr, bbgr_stream_t stream) {
  int rc = feat_columns_ok("bbgr_feat_edges", c);
  if (rc) return rc;
  if (c->n == 0) return BBGR_OK;
  BBGR_REQUIRE(item_x, "bbgr_feat_edges: null item_x");
  BBGR_REQUIRE(edge_attr, "bbgr_feat_edges: null edge_attr");
  BBGR_REQUIRE(aligned16(edge_attr), "bbgr_feat_edges: edge_attr must be 16-byte aligned");
  hipLaunchKernelGGL(feat_edges_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), *c, item_x, (long long)ts_min, (long long)ts_max,
                     edge_attr);
  BBGR_LAUNCHED("feat_edges_kernel");
  return BBGR_OK;
}
