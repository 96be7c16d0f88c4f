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
// inside a group). pool_verify_kernel, one lane per sorted slot, is
// text_verify_kernel's rule with the group in the record's place: a slot opens
// a distinct token when its group or its hash differs from its left
// neighbour's; with both equal the two tokens' normalised bytes are compared
// to their ends and any difference flags the group. A group that owns a record
// bbgr_text_count flagged (U+212A) is flagged too. Integer work only.
//
// bbgr_feat_gaps: days = (ts >= 10^12 ? double(ts) / 1000.0 : double(ts)) /
// 86400.0 per record in the user rows' order (+inf without a timestamp),
// hipcub's segmented radix sort inside each user row, then per user the
// histogram of min(floor(days[j + 1] - days[j]), 365) and its entropy over the
// non-empty bins in ascending order. A row of at most GAP_SHORT_ROW records is
// one lane's: it counts by value (for each distinct bin in ascending order one
// scan of the row), since 366 counters do not fit a lane's registers; a longer
// row is one workgroup's with the histogram in LDS (integer atomics), thread t
// taking bins t and t + 256 and the fixed-shape workgroup sum adding them.
//
// bbgr_feat_users_v2 follows bbgr_feat_users: the same row split at
// FEAT_LONG_ROW, the same fixed-shape double sums, one rounding at the store.
// No fast-math flag on this file: the divisions above must be IEEE double.
//
// Measured in DESIGN 4g (tools/features_bench.py, tools/text_bench.py).
#include "common.h"
#include "features.h"
#include "text.h"

#include <hipcub/hipcub.hpp>

namespace bbgr {

constexpr int GAP_BINS = 366;        // whole days 0 .. 365, the last one the cap
constexpr int GAP_SHORT_ROW = 64;    // records; above: one workgroup and an LDS histogram
constexpr int LENLOG_GRID = 256;     // partial sums of log1p(n_tokens): a fixed grid, a fixed order

// Row bounds of a segmented sort from an indptr: both clamped into [0, n] and
// end >= begin, so no indptr, however wrong, sends the sort outside its keys.
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
  const int lane = threadIdx.x & 63;
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
      TokenCursor a = text_cursor(T, t), b = text_cursor(T, tl);
      for (;;) {
        const int x = a.next(), y = b.next();
        if (x != y) {
          group_recheck[g] = 1;   // every writer stores the same value
          break;
        }
        if (x < 0) break;
      }
    }
  }
  const int left = __shfl_up(g, 1);
  const unsigned long long heads = __ballot(lane == 0 || g != left), open_m = __ballot(opens);
  if (live && (heads >> lane & 1ull)) {
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = after ? __ffsll((long long)after) : 64 - lane;   // lanes of this group here
    const unsigned long long mine = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
    const int cnt = __popcll(open_m & mine);
    if (cnt) atomicAdd(group_unique + g, cnt);
  }
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

__global__ __launch_bounds__(256) void pool_flagged_kernel(int n_groups, const uint8_t *flag,
                                                           long long *totals) {
  long cnt = 0;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (long)gridDim.x * 256)
    cnt += flag[g] != 0;
#pragma unroll
  for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt)
    atomicAdd(reinterpret_cast<unsigned long long *>(totals) + 1, (unsigned long long)cnt);
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
__device__ __forceinline__ double feat2_item_sum(const bbgr_feat_columns &C, const int *eid, int rb,
                                                 int re, int start, int step) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll 4
  for (int p = rb + start; p < re; p += step) s += (double)C.rating[eid[p]];
  return s;
}

__global__ __launch_bounds__(256) void feat2_item_means_kernel(bbgr_feat_columns C,
                                                               const int *indptr, const int *eid,
                                                               double *item_mean, int *long_count,
                                                               int *long_rows, int long_cap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C.n_items) return;
  const int rb = indptr[i], re = indptr[i + 1];
  if (re - rb > FEAT_LONG_ROW) {
    const int pos = atomicAdd(long_count, 1);
    if (pos < long_cap) long_rows[pos] = i;   // always, for an indptr that ends at n
    return;
  }
  const double s = feat2_item_sum(C, eid, rb, re, 0, 1);
  item_mean[i] = re > rb ? s / (double)(re - rb) : 0.0;
}

__global__ __launch_bounds__(256) void feat2_item_means_long_kernel(bbgr_feat_columns C,
                                                                    const int *indptr,
                                                                    const int *eid,
                                                                    double *item_mean,
                                                                    const int *long_count,
                                                                    const int *long_rows,
                                                                    int long_cap) {
  __shared__ double s_d[4];
  const int n_long = min(*long_count, long_cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int i = long_rows[j];
    const int rb = indptr[i], re = indptr[i + 1];
    const double s = feat_block_sum(feat2_item_sum(C, eid, rb, re, threadIdx.x, 256), s_d);
    if (threadIdx.x == 0) item_mean[i] = s / (double)(re - rb);
  }
}

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

__global__ __launch_bounds__(256) void feat2_gaps_kernel(int n_users, RowBound rb_of, RowBound re_of,
                                                         const double *days, double *etg,
                                                         int *long_count, int *long_rows,
                                                         int long_cap) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_users) return;
  const int rb = rb_of(u), re = re_of(u);
  if (re - rb > GAP_SHORT_ROW) {
    const int pos = atomicAdd(long_count, 1);
    if (pos < long_cap) long_rows[pos] = u;   // always: fewer than n / GAP_SHORT_ROW such rows
    return;
  }
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

__global__ __launch_bounds__(256) void feat2_gaps_long_kernel(RowBound rb_of, RowBound re_of,
                                                              const double *days, double *etg,
                                                              const int *long_count,
                                                              const int *long_rows, int long_cap) {
  __shared__ int s_hist[GAP_BINS];
  __shared__ double s_d[4];
  __shared__ int s_i[4];
  const int n_long = min(*long_count, long_cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int u = long_rows[j];
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
    h = feat_block_sum(h, s_d);
    if (threadIdx.x == 0) etg[u] = h;
  }
}

// ---------------------------------------------------------------------------
// Per-user label and the v2 features
// ---------------------------------------------------------------------------
struct UserAcc2 {
  int helpful = 0;
  int h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0;   // histogram of the rounded rating
  int distinct = 0;                             // distinct day buckets
  double ard = 0.0, rd = 0.0;
};

// What the pass needs of a record, in one 16-byte word. x: item, y: n_tokens,
// z: the raw rating's bits, w: ri | 8 when helpful_vote > 5.
__global__ __launch_bounds__(256) void feat2_pack_kernel(bbgr_feat_columns C, int4 *packed) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= C.n) return;
  const float r = C.rating[e];
  packed[e] = make_int4(C.item[e], C.n_tokens[e], __float_as_int(r),
                        feat_ri(r) | (C.helpful_vote[e] > 5 ? 8 : 0));
}

__device__ __forceinline__ void feat2_user_acc(const bbgr_feat_columns &C,
                                               const bbgr_feat_user_v2_args &A,
                                               const int4 *packed, int rb, int re, int bb, int be,
                                               int start, int step, UserAcc2 &a) {
#pragma clang fp contract(off)
#pragma unroll 2
  for (int p = rb + start; p < re; p += step) {
    const int4 r = packed[A.u_eid[p]];
    const int ri = r.w & 7;
    a.h1 += ri == 1;
    a.h2 += ri == 2;
    a.h3 += ri == 3;
    a.h4 += ri == 4;
    a.h5 += ri == 5;
    a.helpful += r.w >> 3;
    const double mean = r.x >= 0 && r.x < C.n_items ? A.item_mean[r.x] : (double)NAN;
    a.ard += fabs((double)__int_as_float(r.z) - mean);
    a.rd += fabs(log1p((double)r.y) - A.global_avg_lenlog);
  }
  for (int p = bb + start; p < be; p += step)
    a.distinct += (p == bb || A.b_bucket[p] != A.b_bucket[p - 1]) ? 1 : 0;
}

__device__ __forceinline__ void feat2_user_store(const bbgr_feat_user_v2_args &A, int u, int n,
                                                 int n_ts, const UserAcc2 &a) {
#pragma clang fp contract(off)
  float *x = A.user_x + 7L * u;
  float *extra = A.user_extra + 2L * u;
  A.total_reviews[u] = n;
  A.helpful_reviews[u] = a.helpful;
  if (n == 0) {   // no record: the NaN row of the graph pass, unlabeled
#pragma unroll
    for (int f = 0; f < 7; ++f) x[f] = NAN;
    extra[0] = NAN;
    extra[1] = NAN;
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
  const long long tokens = A.group_tokens[u];
  x[0] = (float)Ru;
  x[1] = (float)H;
  x[2] = (float)((double)(a.h1 + a.h5) / dn);
  x[3] = (float)(a.ard / dn);
  x[4] = (float)((double)(n_ts - a.distinct) / dn);   // sum over the buckets of (count - 1), / n
  x[5] = tokens > 0 ? (float)((double)A.group_unique[u] / (double)tokens) : 0.f;
  x[6] = (float)(a.rd / dn);
  extra[0] = (float)((double)(a.h1 + a.h2) / dn);
  extra[1] = (float)A.etg[u];
}

__global__ __launch_bounds__(256) void feat2_users_kernel(bbgr_feat_columns C,
                                                          bbgr_feat_user_v2_args A,
                                                          const int4 *packed, int *long_count,
                                                          int *long_rows, int long_cap) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= C.n_users) return;
  const int rb = A.u_indptr[u], re = A.u_indptr[u + 1];
  if (re - rb > FEAT_LONG_ROW) {
    const int pos = atomicAdd(long_count, 1);
    if (pos < long_cap) long_rows[pos] = u;   // always, for an indptr that ends at n
    return;
  }
  const int bb = A.b_indptr[u], be = A.b_indptr[u + 1];
  UserAcc2 a;
  feat2_user_acc(C, A, packed, rb, re, bb, be, 0, 1, a);
  feat2_user_store(A, u, re - rb, be - bb, a);
}

__global__ __launch_bounds__(256) void feat2_users_long_kernel(bbgr_feat_columns C,
                                                               bbgr_feat_user_v2_args A,
                                                               const int4 *packed,
                                                               const int *long_count,
                                                               const int *long_rows,
                                                               int long_cap) {
  __shared__ double s_d[4];
  __shared__ int s_i[4];
  const int n_long = min(*long_count, long_cap);
  for (int j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int u = long_rows[j];
    const int rb = A.u_indptr[u], re = A.u_indptr[u + 1];
    const int bb = A.b_indptr[u], be = A.b_indptr[u + 1];
    UserAcc2 a;
    feat2_user_acc(C, A, packed, rb, re, bb, be, threadIdx.x, 256, a);
    a.helpful = feat_block_sum(a.helpful, s_i);
    a.h1 = feat_block_sum(a.h1, s_i);
    a.h2 = feat_block_sum(a.h2, s_i);
    a.h3 = feat_block_sum(a.h3, s_i);
    a.h4 = feat_block_sum(a.h4, s_i);
    a.h5 = feat_block_sum(a.h5, s_i);
    a.distinct = feat_block_sum(a.distinct, s_i);
    a.ard = feat_block_sum(a.ard, s_d);
    a.rd = feat_block_sum(a.rd, s_d);
    if (threadIdx.x == 0) feat2_user_store(A, u, re - rb, be - bb, a);
  }
}

// The long-row list of a pass that splits at `row`: the counter, then the list.
static size_t feat2_long_bytes(long n, int row) {
  return align_up(256 + sizeof(int) * (size_t)(n / row + 1));
}

}  // namespace bbgr

using namespace bbgr;

#define V2_REQ(fn, cond, what) BBGR_REQUIRE_IN(fn, cond, what)

// bbgr_text_unique_pooled, or (tools/text_bench.py) some of its launch groups
// on a workspace the groups before them have filled.
static int text_unique_pooled(const char *fn, const bbgr_text_args *a, int64_t total_tokens,
                              const int32_t *group, int32_t n_groups, int64_t *group_tokens,
                              int32_t *group_unique, uint8_t *group_recheck, int stages,
                              void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  V2_REQ(fn, a, "null args");
  V2_REQ(fn, n_groups >= 0 && n_groups < INT_MAX, "n_groups out of range (0 <= n_groups < 2^31 - 1)");
  V2_REQ(fn, a->n >= 0 && a->n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  V2_REQ(fn, a->first >= 0 && a->last >= a->first && a->last - a->first < 2147483647LL,
         "first / last out of range (0 <= first <= last, last - first < 2^31 - 1 bytes)");
  V2_REQ(fn, total_tokens >= 0 && total_tokens <= (a->last - a->first + a->n) / 2,
         "total_tokens out of range (at most (last - first + n) / 2)");
  V2_REQ(fn, workspace_bytes, "null workspace_bytes");
  if (a->n > 0) V2_REQ(fn, group, "null group");
  if (a->n > 0 || n_groups > 0) V2_REQ(fn, a->totals, "null totals");
  if (n_groups > 0) {
    V2_REQ(fn, group_tokens, "null group_tokens");
    V2_REQ(fn, group_unique, "null group_unique");
    V2_REQ(fn, group_recheck, "null group_recheck");
  }
  const long n = (long)a->n;
  const int T = (int)total_tokens;
  const size_t nt = (size_t)T;
  // the token stream's own workspace first (its checks of the other fields too)
  size_t base = 0;
  if (int rc = bbgr_text_unique_stages(a, total_tokens, BBGR_TEXT_STAGE_EMIT, nullptr, &base,
                                       stream))
    return rc;
  size_t t_hash = 0, t_group = 0;
  int group_bits = 1;
  while (group_bits < 32 && (unsigned)n_groups >> group_bits) ++group_bits;
  if (T > 0) {
    (void)hipcub::DeviceRadixSort::SortPairs(
        nullptr, t_hash, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
        (const uint32_t *)nullptr, (uint32_t *)nullptr, T, 0, 64, (hipStream_t) nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t_group, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0, group_bits,
                                             (hipStream_t) nullptr);
  }
  const size_t temp = t_hash > t_group ? t_hash : t_group;
  const size_t off_g1 = align_up(base);
  const size_t off_g2 = off_g1 + align_up(sizeof(uint32_t) * nt);
  const size_t off_tmp = off_g2 + align_up(sizeof(uint32_t) * nt);
  const size_t need = off_tmp + align_up(temp);
  if (!workspace) {
    *workspace_bytes = need;
    return BBGR_OK;
  }
  if (*workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", fn, *workspace_bytes, need);
    return BBGR_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (T > 0 && n > 0 && (stages & BBGR_TEXT_STAGE_EMIT)) {
    size_t nb = base;
    if (int rc = bbgr_text_unique_stages(a, total_tokens, BBGR_TEXT_STAGE_EMIT, workspace, &nb,
                                         stream))
      return rc;
  }
  char *ws = static_cast<char *>(workspace);
  const TextWorkspace W = text_workspace(n, nt);
  unsigned long long *k1 = reinterpret_cast<unsigned long long *>(ws + W.off_k1);
  unsigned long long *k2 = reinterpret_cast<unsigned long long *>(ws + W.off_k2);
  uint32_t *v1 = reinterpret_cast<uint32_t *>(ws + W.off_v1);
  uint32_t *v2 = reinterpret_cast<uint32_t *>(ws + W.off_v2);
  uint32_t *g1 = reinterpret_cast<uint32_t *>(ws + off_g1);
  uint32_t *g2 = reinterpret_cast<uint32_t *>(ws + off_g2);
  void *tmp = ws + off_tmp;
  TextTokens K;
  K.n = n;
  K.total = T;
  K.data = a->data;
  K.offsets = reinterpret_cast<const long long *>(a->offsets);
  K.first = (long)a->first;
  K.last = (long)a->last;
  K.tok_pos = reinterpret_cast<const uint32_t *>(ws + W.off_pos);
  K.tok_rec = reinterpret_cast<const int *>(ws + W.off_rec);
  K.tok_off = reinterpret_cast<const int *>(ws);
  K.hash_mask = a->hash_mask ? a->hash_mask : ~0ull;
  const unsigned tok_blocks = (unsigned)(((long)T + 255) / 256);
  if (T > 0 && n > 0 && (stages & BBGR_TEXT_STAGE_SORT)) {
    // by hash, then (stable) by group: equal (group, hash) pairs end side by
    // side, in text order. v1 (the identity before) takes the final order.
    size_t tb = temp;
    BBGR_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const unsigned long long *)k1, k2,
                                                (const uint32_t *)v1, v2, T, 0, 64, st));
    hipLaunchKernelGGL(pool_keys_kernel, dim3(tok_blocks), dim3(256), 0, st, K,
                       (const uint32_t *)v2, group, n_groups, g1);
    BBGR_LAUNCHED("pool_keys_kernel");
    tb = temp;
    BBGR_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const uint32_t *)g1, g2,
                                                (const uint32_t *)v2, v1, T, 0, group_bits, st));
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
  const long gb = ((long)n_groups + 255) / 256;
  hipLaunchKernelGGL(pool_flagged_kernel, dim3((unsigned)(gb < 1024 ? gb : 1024)), dim3(256), 0,
                     st, n_groups, (const uint8_t *)group_recheck,
                     reinterpret_cast<long long *>(a->totals));
  BBGR_LAUNCHED("pool_flagged_kernel");
  return BBGR_OK;
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
  V2_REQ(fn, stages > 0 && stages <= BBGR_TEXT_STAGE_ALL, "stages out of range (1 .. 7)");
  return text_unique_pooled(fn, a, total_tokens, group, n_groups, group_tokens, group_unique,
                            group_recheck, stages, workspace, workspace_bytes, stream);
}

extern "C" int bbgr_feat_lenlog(const bbgr_feat_columns *c, double *lenlog_sum, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_lenlog";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  V2_REQ(fn, workspace_bytes, "null workspace_bytes");
  bool query;
  int rc = feat_workspace(fn, align_up(sizeof(double) * LENLOG_GRID), workspace, workspace_bytes,
                          &query);
  if (rc || query) return rc;
  V2_REQ(fn, lenlog_sum, "null lenlog_sum");
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
  V2_REQ(fn, workspace_bytes, "null workspace_bytes");
  bool query;
  int rc = feat_workspace(fn, feat_long_bytes((long)c->n), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_items == 0) return BBGR_OK;
  V2_REQ(fn, i_indptr, "null i_indptr");
  V2_REQ(fn, c->n == 0 || i_eid, "null i_eid");
  V2_REQ(fn, item_mean, "null item_mean");
  hipStream_t st = as_stream(stream);
  int *long_count = static_cast<int *>(workspace);
  int *long_rows = reinterpret_cast<int *>(static_cast<char *>(workspace) + 256);
  const int long_cap = (int)(c->n / FEAT_LONG_ROW + 1);
  BBGR_HIP(hipMemsetAsync(long_count, 0, sizeof(int), st));
  hipLaunchKernelGGL(feat2_item_means_kernel, dim3((unsigned)((c->n_items + 255) / 256)),
                     dim3(256), 0, st, *c, i_indptr, i_eid, item_mean, long_count, long_rows,
                     long_cap);
  BBGR_LAUNCHED("feat2_item_means_kernel");
  if (c->n > FEAT_LONG_ROW) {
    hipLaunchKernelGGL(feat2_item_means_long_kernel, dim3(FEAT_LONG_GRID), dim3(256), 0, st, *c,
                       i_indptr, i_eid, item_mean, long_count, long_rows, long_cap);
    BBGR_LAUNCHED("feat2_item_means_long_kernel");
  }
  return BBGR_OK;
}

extern "C" int bbgr_feat_gaps(const bbgr_feat_columns *c, const int32_t *u_indptr,
                              const int32_t *u_eid, double *etg, void *workspace,
                              size_t *workspace_bytes, bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_gaps";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  V2_REQ(fn, workspace_bytes, "null workspace_bytes");
  const int n = (int)c->n, U = c->n_users;
  size_t t_sort = 0;
  if (n > 0) {
    const hipcub::CountingInputIterator<int> row(0);
    const RowIter seg_b(row, RowBound{nullptr, n, false}), seg_e(row, RowBound{nullptr, n, true});
    (void)hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, t_sort, (const double *)nullptr,
                                                     (double *)nullptr, n, U, seg_b, seg_e, 0, 64,
                                                     (hipStream_t) nullptr);
  }
  const size_t off_d1 = feat2_long_bytes((long)n, GAP_SHORT_ROW);
  const size_t off_d2 = off_d1 + align_up(sizeof(double) * (size_t)n);
  const size_t off_tmp = off_d2 + align_up(sizeof(double) * (size_t)n);
  bool query;
  int rc = feat_workspace(fn, off_tmp + align_up(t_sort), workspace, workspace_bytes, &query);
  if (rc || query) return rc;
  if (U == 0) return BBGR_OK;
  V2_REQ(fn, u_indptr, "null u_indptr");
  V2_REQ(fn, n == 0 || u_eid, "null u_eid");
  V2_REQ(fn, etg, "null etg");
  hipStream_t st = as_stream(stream);
  char *ws = static_cast<char *>(workspace);
  int *long_count = reinterpret_cast<int *>(ws);
  int *long_rows = reinterpret_cast<int *>(ws + 256);
  const int long_cap = n / GAP_SHORT_ROW + 1;
  double *d1 = reinterpret_cast<double *>(ws + off_d1);
  double *d2 = reinterpret_cast<double *>(ws + off_d2);
  BBGR_HIP(hipMemsetAsync(long_count, 0, sizeof(int), st));
  const RowBound rb_of{u_indptr, n, false}, re_of{u_indptr, n, true};
  if (n > 0) {
    hipLaunchKernelGGL(feat2_days_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *c,
                       u_eid, d1);
    BBGR_LAUNCHED("feat2_days_kernel");
    const hipcub::CountingInputIterator<int> row(0);
    const RowIter seg_b(row, rb_of), seg_e(row, re_of);
    size_t tb = t_sort;
    BBGR_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(ws + off_tmp, tb, (const double *)d1, d2,
                                                        n, U, seg_b, seg_e, 0, 64, st));
  }
  hipLaunchKernelGGL(feat2_gaps_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, st, U,
                     rb_of, re_of, (const double *)d2, etg, long_count, long_rows, long_cap);
  BBGR_LAUNCHED("feat2_gaps_kernel");
  if (n > GAP_SHORT_ROW) {
    hipLaunchKernelGGL(feat2_gaps_long_kernel, dim3(FEAT_LONG_GRID), dim3(256), 0, st, rb_of,
                       re_of, (const double *)d2, etg, (const int *)long_count,
                       (const int *)long_rows, long_cap);
    BBGR_LAUNCHED("feat2_gaps_long_kernel");
  }
  return BBGR_OK;
}

extern "C" int bbgr_feat_users_v2(const bbgr_feat_columns *c, const bbgr_feat_user_v2_args *a,
                                  void *workspace, size_t *workspace_bytes,
                                  bbgr_stream_t stream) {
  static const char *fn = "bbgr_feat_users_v2";
  if (int rc = feat_columns_ok(fn, c)) return rc;
  V2_REQ(fn, a, "null args");
  V2_REQ(fn, workspace_bytes, "null workspace_bytes");
  bool query;
  // the long-row list, then the packed records
  const size_t off_packed = feat_long_bytes((long)c->n);
  int rc = feat_workspace(fn, off_packed + align_up(sizeof(int4) * (size_t)c->n), workspace,
                          workspace_bytes, &query);
  if (rc || query) return rc;
  if (c->n_users == 0) return BBGR_OK;
  V2_REQ(fn, a->u_indptr, "null u_indptr");
  V2_REQ(fn, a->b_indptr, "null b_indptr");
  if (c->n > 0) {
    V2_REQ(fn, a->u_eid, "null u_eid");
    V2_REQ(fn, a->b_bucket, "null b_bucket");
    V2_REQ(fn, a->item_mean, "null item_mean");
  }
  V2_REQ(fn, a->group_tokens, "null group_tokens");
  V2_REQ(fn, a->group_unique, "null group_unique");
  V2_REQ(fn, a->etg, "null etg");
  V2_REQ(fn, a->user_x, "null user_x");
  V2_REQ(fn, a->user_y, "null user_y");
  V2_REQ(fn, a->total_reviews, "null total_reviews");
  V2_REQ(fn, a->helpful_reviews, "null helpful_reviews");
  V2_REQ(fn, a->user_extra, "null user_extra");
  hipStream_t st = as_stream(stream);
  int *long_count = static_cast<int *>(workspace);
  int *long_rows = reinterpret_cast<int *>(static_cast<char *>(workspace) + 256);
  const int long_cap = (int)(c->n / FEAT_LONG_ROW + 1);
  BBGR_HIP(hipMemsetAsync(long_count, 0, sizeof(int), st));
  int4 *packed = reinterpret_cast<int4 *>(static_cast<char *>(workspace) + off_packed);
  if (c->n > 0) {
    hipLaunchKernelGGL(feat2_pack_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, st,
                       *c, packed);
    BBGR_LAUNCHED("feat2_pack_kernel");
  }
  hipLaunchKernelGGL(feat2_users_kernel, dim3((unsigned)((c->n_users + 255) / 256)), dim3(256), 0,
                     st, *c, *a, packed, long_count, long_rows, long_cap);
  BBGR_LAUNCHED("feat2_users_kernel");
  if (c->n > FEAT_LONG_ROW) {
    hipLaunchKernelGGL(feat2_users_long_kernel, dim3(FEAT_LONG_GRID), dim3(256), 0, st, *c, *a,
                       packed, long_count, long_rows, long_cap);
    BBGR_LAUNCHED("feat2_users_long_kernel");
  }
  return BBGR_OK;
}
