// The second feature pipeline (main_v2_.py:291-524): per user the pooled
// distinct-token count, the entropy of the gaps between review times (ETG),
// the share of low ratings (RNR), and the four behavioural columns whose
// definition differs from main.py's (features.hip).
//
// bbgr_text_unique_pooled: distinct normalised tokens over ALL records of a
// group (the user). The token stream is the one bbgr_text_unique's EMIT stage
// leaves in its workspace: per token its record, its start and its 64-bit
// hash (text.hip; the same rule, the same hash, the same mask). Two stable
// radix sorts bring equal (group, hash) pairs side by side: all tokens by
// hash, then by group over the bits n_groups needs (the hash order survives
// inside a group). pool_verify_kernel, one lane per sorted slot, applies
// text_verify_kernel's rule (text.h: the comparison, the count per wave) with
// the group in the record's place: a slot opens a distinct token when its
// group or its hash differs from its left neighbour's; with both equal the two
// tokens' normalised bytes are compared to their ends and any difference flags
// the group. A group that owns a record bbgr_text_count flagged (U+212A) is
// flagged too. Integer work only.
//
// bbgr_feat_gaps: days = (ts >= 10^12 ? double(ts) / 1000.0 : double(ts)) /
// 86400.0 per record in the user rows' order (+inf without a timestamp),
// hipcub's segmented radix sort inside each user row, then per user the
// histogram of min(floor(days[j + 1] - days[j]), 365) and its entropy over the
// non-empty bins in ascending order. GapsPass runs through features.h's row
// pass with its own limit: a row of at most GAP_SHORT_ROW records is one
// lane's, which counts by value (for each distinct bin in ascending order one
// scan of the row), since 366 counters do not fit a lane's registers; a longer
// row is one workgroup's with the histogram in LDS (integer atomics), thread t
// taking bins t and t + 256 and the fixed-shape workgroup sum adding them.
//
// ItemMeansPass and UsersV2Pass are sum passes of features.h like
// features.hip's two; the user pass shares its counts, its label and columns
// 0 to 2 with bbgr_feat_users' and adds its own two double sums and columns.
// No fast-math flag on this file: the divisions above must be IEEE double.
//
// Measured in DESIGN 4g (tools/features_bench.py, tools/text_bench.py).
#include "cub_temp.h"
#include "features.h"
#include "text.h"


namespace bbgr {

constexpr int GAP_BINS = 366;        // whole days 0 .. 365, the last one the cap
constexpr int GAP_SHORT_ROW = 64;    // records; above: one workgroup and an LDS histogram
constexpr int LENLOG_GRID = 256;     // partial sums of log1p(n_tokens): a fixed grid, a fixed order

typedef hipcub::TransformInputIterator<int, RowBound, hipcub::CountingInputIterator<int>> RowIter;

// ---------------------------------------------------------------------------
// Pooled distinct tokens per group
// ---------------------------------------------------------------------------
// The group of every slot of the hash-sorted stream; n_groups (a spare key,
// sorted last, which nothing counts) for a slot whose token, record or group
// is out of range.
__global__ __launch_bounds__(256) void pool_keys_kernel(TextTokens T, const uint32_t *vals,
                                                        const int *group, int n_groups,
                                                        uint32_t *gkey) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= T.total) return;
  int g = n_groups;
  const long t = (long)vals[j];
  if (t < text_live_tokens(T)) {
    const int rec = T.tok_rec[t];
    if (rec >= 0 && rec < T.n) {
      const int gg = group[rec];
      if (gg >= 0 && gg < n_groups) g = gg;
    }
  }
  gkey[j] = (uint32_t)g;
}

// One lane per slot of the (group, hash)-sorted stream. hash: by token index.
// group_unique was zeroed; the lanes of a wave that share a group add their
// count with one integer atomic.
__global__ __launch_bounds__(256) void pool_verify_kernel(TextTokens T,
                                                          const unsigned long long *hash,
                                                          const uint32_t *gkey,
                                                          const uint32_t *vals, int n_groups,
                                                          int *group_unique,
                                                          uint8_t *group_recheck) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const long live_tokens = text_live_tokens(T);
  int g = -1;
  long t = 0;
  if (j < T.total) {
    const uint32_t gg = gkey[j];
    t = (long)vals[j];
    if (gg < (uint32_t)n_groups && t < live_tokens) g = (int)gg;
  }
  const bool live = g >= 0;
  bool opens = live;
  if (live && j > 0) {
    const long tl = (long)vals[j - 1];
    if (gkey[j - 1] == (uint32_t)g && tl < live_tokens && hash[tl] == hash[t]) {
      opens = false;
      if (text_tokens_differ(T, t, tl)) group_recheck[g] = 1;   // every writer stores the same value
    }
  }
  text_count_opens(g, live, opens, group_unique);
}

// Per record: its tokens to its group's total, its U+212A flag to its group.
__global__ __launch_bounds__(256) void pool_records_kernel(long n, const int *n_tokens,
                                                           const uint8_t *recheck,
                                                           const int *group, int n_groups,
                                                           unsigned long long *group_tokens,
                                                           uint8_t *group_recheck) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int g = group[r];
  if (g < 0 || g >= n_groups) return;
  const int L = n_tokens[r];
  if (L > 0) atomicAdd(group_tokens + g, (unsigned long long)L);
  if (recheck[r]) group_recheck[g] = 1;
}

// ---------------------------------------------------------------------------
// Sum of log1p(n_tokens) in double: LENLOG_GRID partial sums, each thread its
// records e, e + grid * 256, .. in order, then one workgroup adds the partials.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat2_lenlog_kernel(long n, const int *n_tokens,
                                                           double *partial) {
#pragma clang fp contract(off)
  __shared__ double s_d[4];
  double v = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)LENLOG_GRID * 256)
    v += log1p((double)n_tokens[e]);
  v = feat_block_sum(v, s_d);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void feat2_lenlog_final_kernel(const double *partial,
                                                                 double *out) {
  __shared__ double s_d[4];
  static_assert(LENLOG_GRID == 256, "one partial a thread");
  const double v = feat_block_sum(partial[threadIdx.x], s_d);
  if (threadIdx.x == 0) out[0] = v;
}

// ---------------------------------------------------------------------------
// Per item the double mean of the raw rating (item_sum[item] += r_ui in file
// order for a short row; 0 for an item with no record)
// ---------------------------------------------------------------------------
struct ItemMeansPass : SumPass<ItemMeansPass> {
  bbgr_feat_columns C;
  const int *eid;
  double *item_mean;
  struct Acc {
    double s = 0.0;
    __device__ __forceinline__ void block_sum() {
      __shared__ double s_d[4];
      s = feat_block_sum(s, s_d);
    }
  };
  __device__ __forceinline__ void accumulate(int i, int start, int step, Acc &a) const {
#pragma clang fp contract(off)
    const int re = indptr[i + 1];
#pragma unroll 4
    for (int p = indptr[i] + start; p < re; p += step) a.s += (double)C.rating[eid[p]];
  }
  // n > 0 in a long row, which therefore divides as it always did
  __device__ __forceinline__ void store(int i, int n, const Acc &a) const {
#pragma clang fp contract(off)
    item_mean[i] = n > 0 ? a.s / (double)n : 0.0;
  }
};

// ---------------------------------------------------------------------------
// Gap entropy
// ---------------------------------------------------------------------------
// ts_to_days(): both divisions IEEE double, in this order.
__device__ __forceinline__ double feat2_days(long long ts) {
#pragma clang fp contract(off)
  double s = (double)ts;
  if (ts >= 1000000000000LL) s = s / 1000.0;
  return s / 86400.0;
}

__global__ __launch_bounds__(256) void feat2_days_kernel(bbgr_feat_columns C, const int *u_eid,
                                                         double *days) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= C.n) return;
  const int e = u_eid[p];
  const bool ok = e >= 0 && e < C.n && feat_has_ts(C, e);
  days[p] = ok ? feat2_days(C.timestamp[e]) : (double)INFINITY;
}

// The bin of the gap after sorted slot p (p + 1 holds a finite day too).
__device__ __forceinline__ int feat2_gap_bin(const double *days, int p) {
#pragma clang fp contract(off)
  const double gap = days[p + 1] - days[p];
  return (int)fmin(floor(gap), (double)(GAP_BINS - 1));
}

// A row pass of its own shape: the rows are the sorted days of a user, by the
// clamped bounds the sort used.
struct GapsPass {
  static constexpr int LONG_ROW = GAP_SHORT_ROW;
  const int *indptr;
  int n;
  const double *days;
  double *etg;
  __device__ __forceinline__ int rb_of(int u) const { return RowBound{indptr, n, false}(u); }
  __device__ __forceinline__ int re_of(int u) const { return RowBound{indptr, n, true}(u); }
  __device__ __forceinline__ int length(int u) const { return re_of(u) - rb_of(u); }
  __device__ __forceinline__ void short_row(int u) const {
    const int rb = rb_of(u), re = re_of(u);
    int m = 0;   // the finite days are the row's first m: +inf sorts last
    while (rb + m < re && days[rb + m] < (double)INFINITY) ++m;
    double H = 0.0;
    if (m >= 3) {
      const int gaps = m - 1;
      for (int cur = -1;;) {   // the distinct bins in ascending order, one scan each
        int next = INT_MAX, cnt = 0;
        for (int j = 0; j < gaps; ++j) {
          const int b = feat2_gap_bin(days, rb + j);
          if (b > cur && b <= next) {
            cnt = b < next ? 1 : cnt + 1;
            next = b;
          }
        }
        if (next == INT_MAX) break;
        H = feat_plogp(H, cnt, (double)gaps);
        cur = next;
      }
    }
    etg[u] = H;
  }
  __device__ __forceinline__ void long_row(int u) const {
    __shared__ int s_hist[GAP_BINS];
    __shared__ double s_d[4];
    __shared__ int s_i[4];
    const int rb = rb_of(u), re = re_of(u);
    for (int b = threadIdx.x; b < GAP_BINS; b += 256) s_hist[b] = 0;
    int fin = 0;
    for (int p = rb + threadIdx.x; p < re; p += 256) fin += days[p] < (double)INFINITY ? 1 : 0;
    const int m = feat_block_sum(fin, s_i);   // its barriers also publish the zeroed histogram
    const int gaps = m - 1;
    if (m >= 3)
      for (int g = threadIdx.x; g < gaps; g += 256) atomicAdd(&s_hist[feat2_gap_bin(days, rb + g)], 1);
    __syncthreads();
    double h = 0.0;
    if (m >= 3)
      for (int b = threadIdx.x; b < GAP_BINS; b += 256) h = feat_plogp(h, s_hist[b], (double)gaps);
    h = feat_block_sum(h, s_d);   // and its last barrier frees the histogram for the next row
    if (threadIdx.x == 0) etg[u] = h;
  }
};

// ---------------------------------------------------------------------------
// Per-user label and the v2 features: features.h's user pass with
// main_v2_.py's two double sums, its columns 3 to 6 and user_extra
// ---------------------------------------------------------------------------
struct UsersV2Pass : SumPass<UsersV2Pass> {
  bbgr_feat_columns C;
  bbgr_feat_user_v2_args A;
  const int4 *packed;   // feat_pack_kernel<true>: z is the raw rating's bits
  struct Acc : UserCounts {
    double ard = 0.0, rd = 0.0;
    __device__ __forceinline__ void block_sum() {
      __shared__ double s_d[4];
      UserCounts::block_sum();
      ard = feat_block_sum(ard, s_d);
      rd = feat_block_sum(rd, s_d);
    }
  };
  __device__ __forceinline__ void accumulate(int u, int start, int step, Acc &a) const {
#pragma clang fp contract(off)
    const int re = indptr[u + 1];
#pragma unroll 2
    for (int p = indptr[u] + start; p < re; p += step) {
      const int4 r = packed[A.u_eid[p]];
      a.add(r.w);
      const double mean = r.x >= 0 && r.x < C.n_items ? A.item_mean[r.x] : (double)NAN;
      a.ard += fabs((double)__int_as_float(r.z) - mean);
      a.rd += fabs(log1p((double)r.y) - A.global_avg_lenlog);
    }
    a.add_buckets(A.b_indptr, A.b_bucket, u, start, step);
  }
  __device__ __forceinline__ void store(int u, int n, const Acc &a) const {
#pragma clang fp contract(off)
    float *x = A.user_x + 7L * u;
    float *extra = A.user_extra + 2L * u;
    if (!feat_user_head(A, u, n, a)) {
      extra[0] = NAN;
      extra[1] = NAN;
      return;
    }
    const double dn = (double)n;
    const long long tokens = A.group_tokens[u];
    x[3] = (float)(a.ard / dn);
    x[4] = (float)((double)(a.n_ts - a.distinct) / dn);   // sum over the buckets of (count - 1), / n
    x[5] = tokens > 0 ? (float)((double)A.group_unique[u] / (double)tokens) : 0.f;
    x[6] = (float)(a.rd / dn);
    extra[0] = (float)((double)(a.h1 + a.h2) / dn);
    extra[1] = (float)A.etg[u];
  }
};

}  // namespace bbgr

using namespace bbgr;

// bbgr_text_unique_pooled, or (tools/text_bench.py) some of its launch groups
// on a workspace the groups before them have filled.
static int text_unique_pooled(const char *fn, const bbgr_text_args *a, int64_t total_tokens,
                              const int32_t *group, int32_t n_groups, int64_t *group_tokens,
                              int32_t *group_unique, uint8_t *group_recheck, int stages,
                              void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  BBGR_REQUIRE_IN(fn, a, "null args");
  BBGR_REQUIRE_IN(fn, n_groups >= 0 && n_groups < INT_MAX,
                  "n_groups out of range (0 <= n_groups < 2^31 - 1)");
  // text_check's three range checks of first and last in this entry's one wording
  BBGR_REQUIRE_IN(fn, a->first >= 0 && a->last >= a->first && a->last - a->first < 2147483647LL,
                  "first / last out of range (0 <= first <= last, last - first < 2^31 - 1 bytes)");
  if (int rc = text_check(fn, a)) return rc;
  BBGR_REQUIRE_IN(fn, total_tokens >= 0 && total_tokens <= (a->last - a->first + a->n) / 2,
                  "total_tokens out of range (at most (last - first + n) / 2)");
  if (a->n > 0) BBGR_REQUIRE_IN(fn, group, "null group");
  if (n_groups > 0) {
    BBGR_REQUIRE_IN(fn, a->totals, "null totals");
    BBGR_REQUIRE_IN(fn, group_tokens, "null group_tokens");
    BBGR_REQUIRE_IN(fn, group_unique, "null group_unique");
    BBGR_REQUIRE_IN(fn, group_recheck, "null group_recheck");
  }
  const long n = (long)a->n;
  const int T = (int)total_tokens;
  const size_t nt = (size_t)T;
  // the token stream's own workspace first
  size_t base = 0;
  if (int rc = bbgr_text_unique_stages(a, total_tokens, BBGR_TEXT_STAGE_EMIT, nullptr, &base,
                                       stream))
    return rc;
  size_t t_hash = 0, t_group = 0;
  int group_bits = 1;
  while (group_bits < 32 && (unsigned)n_groups >> group_bits) ++group_bits;
  if (T > 0) {
    t_hash = hcub::sort_pairs_temp<unsigned long long, uint32_t>(T, 0, 64);
    t_group = hcub::sort_pairs_temp<uint32_t, uint32_t>(T, 0, group_bits);
  }
  const size_t temp = t_hash > t_group ? t_hash : t_group;
  Carver C;
  C.take(base);
  const size_t off_g1 = C.take_n<uint32_t>(nt), off_g2 = C.take_n<uint32_t>(nt);
  const size_t off_tmp = C.take(temp);
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  hipStream_t st = as_stream(stream);
  if (T > 0 && n > 0 && (stages & BBGR_TEXT_STAGE_EMIT)) {
    size_t nb = base;
    rc = bbgr_text_unique_stages(a, total_tokens, BBGR_TEXT_STAGE_EMIT, workspace, &nb, stream);
    if (rc) return rc;
  }
  const TextWorkspace W = text_workspace(n, nt);
  unsigned long long *k1 = ws_at<unsigned long long>(workspace, W.off_k1);
  unsigned long long *k2 = ws_at<unsigned long long>(workspace, W.off_k2);
  uint32_t *v1 = ws_at<uint32_t>(workspace, W.off_v1), *v2 = ws_at<uint32_t>(workspace, W.off_v2);
  uint32_t *g1 = ws_at<uint32_t>(workspace, off_g1), *g2 = ws_at<uint32_t>(workspace, off_g2);
  void *tmp = ws_at<char>(workspace, off_tmp);
  const TextTokens K = text_tokens(a, workspace, W, T);
  const unsigned tok_blocks = (unsigned)(((long)T + 255) / 256);
  if (T > 0 && n > 0 && (stages & BBGR_TEXT_STAGE_SORT)) {
    // by hash, then (stable) by group: equal (group, hash) pairs end side by
    // side, in text order. v1 (the identity before) takes the final order.
    BBGR_HIP(hcub::sort_pairs(tmp, temp, (const unsigned long long *)k1, k2, (const uint32_t *)v1,
                              v2, T, 0, 64, st));
    hipLaunchKernelGGL(pool_keys_kernel, dim3(tok_blocks), dim3(256), 0, st, K,
                       (const uint32_t *)v2, group, n_groups, g1);
    BBGR_LAUNCHED("pool_keys_kernel");
    BBGR_HIP(hcub::sort_pairs(tmp, temp, (const uint32_t *)g1, g2, (const uint32_t *)v2, v1, T, 0,
                              group_bits, st));
  }
  if (!(stages & BBGR_TEXT_STAGE_VERIFY)) return BBGR_OK;
  if (n_groups > 0) {
    BBGR_HIP(hipMemsetAsync(group_tokens, 0, sizeof(int64_t) * (size_t)n_groups, st));
    BBGR_HIP(hipMemsetAsync(group_unique, 0, sizeof(int32_t) * (size_t)n_groups, st));
    BBGR_HIP(hipMemsetAsync(group_recheck, 0, (size_t)n_groups, st));
  }
  if (a->totals) BBGR_HIP(hipMemsetAsync(a->totals + 1, 0, sizeof(int64_t), st));
  if (n == 0 || n_groups == 0) return BBGR_OK;
  if (T > 0) {
    // the hashes by token index: k1 is the first sort's input, left as it was
    hipLaunchKernelGGL(pool_verify_kernel, dim3(tok_blocks), dim3(256), 0, st, K,
                       (const unsigned long long *)k1, (const uint32_t *)g2, (const uint32_t *)v1,
                       n_groups, group_unique, group_recheck);
    BBGR_LAUNCHED("pool_verify_kernel");
  }
  hipLaunchKernelGGL(pool_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                     (const int *)a->n_tokens, (const uint8_t *)a->recheck, group, n_groups,
                     reinterpret_cast<unsigned long long *>(group_tokens), group_recheck);
  BBGR_LAUNCHED("pool_records_kernel");
  return text_flag_total((long)n_groups, group_recheck, a->totals, st);
}

extern "C" int bbgr_text_unique_pooled(const bbgr_text_args *a, int64_t total_tokens,
                                       const int32_t *group, int32_t n_groups,
                                       int64_t *group_tokens, int32_t *group_unique,
                                       uint8_t *group_recheck, void *workspace,
                                       size_t *workspace_bytes, bbgr_stream_t stream) {
  return text_unique_pooled("bbgr_text_unique_pooled", a, total_tokens, group, n_groups,
                            group_tokens, group_unique, group_recheck, BBGR_TEXT_STAGE_ALL,
                            workspace, workspace_bytes, stream);
}

extern "C" int bbgr_text_unique_pooled_stages(const bbgr_text_args *a, int64_t total_tokens,
                                              const int32_t *group, int32_t n_groups,
                                              int64_t *group_tokens, int32_t *group_unique,
                                              uint8_t *group_recheck, int32_t stages,
                                              void *workspace, size_t *workspace_bytes,
                                              bbgr_stream_t stream) {
  static const char *fn = "bbgr_text_unique_pooled_stages";
  BBGR_REQUIRE_IN(fn, stages > 0 && stages <= BBGR_TEXT_STAGE_ALL, "stages out of range (1 .. 7)");
  return text_unique_pooled(fn, a, total_tokens, group, n_groups, group_tokens, group_unique,
                            group_recheck, stages, workspace, workspace_bytes, stream);
}

extern "C" int bbgr_feat_lenlog(const bbgr_feat_columns *c, double *lenlog_sum, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_lenlog";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  bool query;
  int rc = take_workspace(fn, align_up(sizeof(double) * LENLOG_GRID), workspace, workspace_bytes,
                          &query);
  if (rc || query) return rc;
  BBGR_REQUIRE_IN(fn, lenlog_sum, "null lenlog_sum");
  hipStream_t st = as_stream(stream);
  double *partial = static_cast<double *>(workspace);
  hipLaunchKernelGGL(feat2_lenlog_kernel, dim3(LENLOG_GRID), dim3(256), 0, st, (long)c->n,
                     (const int *)c->n_tokens, partial);
  BBGR_LAUNCHED("feat2_lenlog_kernel");
  hipLaunchKernelGGL(feat2_lenlog_final_kernel, dim3(1), dim3(256), 0, st,
                     (const double *)partial, lenlog_sum);
  BBGR_LAUNCHED("feat2_lenlog_final_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_feat_item_means(const bbgr_feat_columns *c, const int32_t *i_indptr,
                                    const int32_t *i_eid, double *item_mean, void *workspace,
                                    size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_item_means";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  bool query;
  int rc = take_workspace(fn, feat_long_bytes((long)c->n), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_items == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, i_indptr, "null i_indptr");
  BBGR_REQUIRE_IN(fn, c->n == 0 || i_eid, "null i_eid");
  BBGR_REQUIRE_IN(fn, item_mean, "null item_mean");
  return feat_row_pass(fn, ItemMeansPass{{i_indptr}, *c, i_eid, item_mean}, c->n_items, (long)c->n,
                       workspace, as_stream(stream));
}

extern "C" int bbgr_feat_gaps(const bbgr_feat_columns *c, const int32_t *u_indptr,
                              const int32_t *u_eid, double *etg, void *workspace,
                              size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_gaps";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  const int n = (int)c->n, U = c->n_users;
  size_t t_sort = 0;
  if (n > 0) {
    const hipcub::CountingInputIterator<int> row(0);
    const RowIter seg_b(row, RowBound{nullptr, n, false}), seg_e(row, RowBound{nullptr, n, true});
    t_sort = hcub::seg_sort_keys_temp<double>(n, U, seg_b, seg_e, 0, 64);
  }
  // the long-row list, the day keys before and after the sort, the sort's temp
  Carver C;
  C.take(feat_long_bytes((long)n, GAP_SHORT_ROW));
  const size_t off_d1 = C.take_n<double>((size_t)n), off_d2 = C.take_n<double>((size_t)n);
  const size_t off_tmp = C.take(t_sort);
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (U == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, u_indptr, "null u_indptr");
  BBGR_REQUIRE_IN(fn, n == 0 || u_eid, "null u_eid");
  BBGR_REQUIRE_IN(fn, etg, "null etg");
  hipStream_t st = as_stream(stream);
  double *d1 = ws_at<double>(workspace, off_d1), *d2 = ws_at<double>(workspace, off_d2);
  const RowBound rb_of{u_indptr, n, false}, re_of{u_indptr, n, true};
  if (n > 0) {
    hipLaunchKernelGGL(feat2_days_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *c,
                       u_eid, d1);
    BBGR_LAUNCHED("feat2_days_kernel");
    const hipcub::CountingInputIterator<int> row(0);
    const RowIter seg_b(row, rb_of), seg_e(row, re_of);
    BBGR_HIP(hcub::seg_sort_keys(ws_at<char>(workspace, off_tmp), t_sort, (const double *)d1, d2,
                                 n, U, seg_b, seg_e, 0, 64, st));
  }
  return feat_row_pass(fn, GapsPass{u_indptr, n, d2, etg}, U, (long)n, workspace, st);
}

extern "C" int bbgr_feat_users_v2(const bbgr_feat_columns *c, const bbgr_feat_user_v2_args *a,
                                  void *workspace, size_t *workspace_bytes,
                                  bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_users_v2";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  BBGR_REQUIRE_IN(fn, a, "null args");
  bool query;
  // the long-row list, then the packed records
  Carver C;
  C.take(feat_long_bytes((long)c->n));
  const size_t off_packed = C.take_n<int4>((size_t)c->n);
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_users == 0) return BBGR_OK;
  BBGR_REQUIRE_IN(fn, a->u_indptr, "null u_indptr");
  BBGR_REQUIRE_IN(fn, a->b_indptr, "null b_indptr");
  if (c->n > 0) {
    BBGR_REQUIRE_IN(fn, a->u_eid, "null u_eid");
    BBGR_REQUIRE_IN(fn, a->b_bucket, "null b_bucket");
    BBGR_REQUIRE_IN(fn, a->item_mean, "null item_mean");
  }
  BBGR_REQUIRE_IN(fn, a->group_tokens, "null group_tokens");
  BBGR_REQUIRE_IN(fn, a->group_unique, "null group_unique");
  BBGR_REQUIRE_IN(fn, a->etg, "null etg");
  BBGR_REQUIRE_IN(fn, a->user_x, "null user_x");
  BBGR_REQUIRE_IN(fn, a->user_y, "null user_y");
  BBGR_REQUIRE_IN(fn, a->total_reviews, "null total_reviews");
  BBGR_REQUIRE_IN(fn, a->helpful_reviews, "null helpful_reviews");
  BBGR_REQUIRE_IN(fn, a->user_extra, "null user_extra");
  hipStream_t st = as_stream(stream);
  int4 *packed = ws_at<int4>(workspace, off_packed);
  if ((rc = feat_pack<true>(c, packed, st))) return rc;
  return feat_row_pass(fn, UsersV2Pass{{a->u_indptr}, *c, *a, packed}, c->n_users, (long)c->n,
                       workspace, st);
}
