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
// The two row passes (ItemsPass, UsersPass) say only what a record adds and
// what a row stores; features.h's row pass runs them: a row of at most
// FEAT_LONG_ROW records is summed by one lane in file order (the order of the
// reference's loops), a longer row by one workgroup in a fixed shape. Every
// sum is taken in double, without float atomics, and rounded to float once, at
// the store.
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
struct ItemsPass : SumPass<ItemsPass> {
  bbgr_feat_columns C;
  const int *eid;
  float *item_x;
  double *item_rbar;
  struct Acc {
    double sum_r = 0.0;
    long long sum_ri = 0;
    __device__ __forceinline__ void block_sum() {
      __shared__ double s_d[4];
      __shared__ long long s_l[4];
      sum_r = feat_block_sum(sum_r, s_d);
      sum_ri = feat_block_sum(sum_ri, s_l);
    }
  };
  __device__ __forceinline__ void accumulate(int i, int start, int step, Acc &a) const {
#pragma clang fp contract(off)
    const int re = indptr[i + 1];
#pragma unroll 4
    for (int p = indptr[i] + start; p < re; p += step) {
      const float r = C.rating[eid[p]];
      a.sum_r += (double)r;
      a.sum_ri += feat_ri(r);
    }
  }
  __device__ __forceinline__ void store(int i, int n, const Acc &a) const {
#pragma clang fp contract(off)
    const double den = n > 0 ? (double)n : 1.0;
    item_x[2L * i] = (float)(a.sum_r / den);
    item_x[2L * i + 1] = (float)n;
    item_rbar[i] = (double)a.sum_ri / den;
  }
};

// ---------------------------------------------------------------------------
// Per-user label and features: features.h's user pass with main.py's three
// double sums and its columns 3 to 6
// ---------------------------------------------------------------------------
struct UsersPass : SumPass<UsersPass> {
  bbgr_feat_columns C;
  bbgr_feat_user_args A;
  const int4 *packed;   // feat_pack_kernel<false>: z is n_unique_tokens
  struct Acc : UserCounts {
    double aad = 0.0, ld = 0.0, rd = 0.0;
    __device__ __forceinline__ void block_sum() {
      __shared__ double s_d[4];
      UserCounts::block_sum();
      aad = feat_block_sum(aad, s_d);
      ld = feat_block_sum(ld, s_d);
      rd = feat_block_sum(rd, s_d);
    }
  };
  __device__ __forceinline__ void accumulate(int u, int start, int step, Acc &a) const {
#pragma clang fp contract(off)
    const int re = indptr[u + 1];
#pragma unroll 4
    for (int p = indptr[u] + start; p < re; p += step) {
      const int4 r = packed[A.u_eid[p]];
      a.add(r.w);
      const double rbar = r.x >= 0 && r.x < C.n_items ? A.item_rbar[r.x] : (double)NAN;
      a.aad += fabs((double)(r.w & 7) - rbar);
      const int L = r.y;
      if (L > 0) a.ld += (double)r.z / (double)L;
      a.rd += fabs((double)L - A.global_avg_len);
    }
    a.add_buckets(A.b_indptr, A.b_bucket, u, start, step);
  }
  __device__ __forceinline__ void store(int u, int n, const Acc &a) const {
#pragma clang fp contract(off)
    if (!feat_user_head(A, u, n, a)) return;
    const double dn = (double)n;
    float *x = A.user_x + 7L * u;
    x[3] = (float)(a.aad / dn);
    x[4] = (float)(a.n_ts - a.distinct);   // sum over the buckets of (count - 1)
    x[5] = (float)(a.ld / dn);
    x[6] = (float)(a.rd / dn);
  }
};

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
  static const char *fn = "bbgr_feat_items";
  int rc = feat_columns_ok(fn, c);
  if (rc) return rc;
  bool query;
  rc = take_workspace(fn, feat_long_bytes((long)c->n), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_items == 0) return BBGR_OK;
  BBGR_REQUIRE(i_indptr, "bbgr_feat_items: null i_indptr");
  BBGR_REQUIRE(c->n == 0 || i_eid, "bbgr_feat_items: null i_eid");
  BBGR_REQUIRE(item_x, "bbgr_feat_items: null item_x");
  BBGR_REQUIRE(item_rbar, "bbgr_feat_items: null item_rbar");
  return feat_row_pass(fn, ItemsPass{{i_indptr}, *c, i_eid, item_x, item_rbar}, c->n_items,
                       (long)c->n, workspace, as_stream(stream));
}

extern "C" int bbgr_feat_users(const bbgr_feat_columns *c, const bbgr_feat_user_args *a,
                               void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_users";
  int rc = feat_columns_ok(fn, c);
  if (rc) return rc;
  BBGR_REQUIRE(a, "bbgr_feat_users: null args");
  bool query;
  // the long-row list, then the packed records
  Carver C;
  C.take(feat_long_bytes((long)c->n));
  const size_t off_packed = C.take_n<int4>((size_t)c->n);
  rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
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
  int4 *packed = ws_at<int4>(workspace, off_packed);
  if ((rc = feat_pack<false>(c, packed, st))) return rc;
  return feat_row_pass(fn, UsersPass{{a->u_indptr}, *c, *a, packed}, c->n_users, (long)c->n,
                       workspace, st);
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
