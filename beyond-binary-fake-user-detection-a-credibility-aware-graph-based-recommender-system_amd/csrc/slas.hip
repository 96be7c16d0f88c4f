// SLAS subgraph sampling for the credibility GNN (main.py:727-883): the
// similarity profiles, the weighted without-replacement neighbour sample of a
// list of rows, and the induced edge list of a sampled user / item set.
//
// All three walk the reference-order CSR (build_csr_from_src, main.py:739-749:
// a stable sort by source, so a row lists its edges by ascending input edge
// id), given as indptr + neighbour id per slot + edge id per slot.
//
// The sampler draws by exponential clocks: slot j of a row gets the key
// -log(U_j) / w_j, the k smallest keys are the sample, in ascending key order.
// That is successive sampling with probabilities proportional to w, the
// distribution of rng.choice(m, k, replace=False, p=w/sum(w)). One wave owns a
// row; lane j holds the j-th smallest (key, slot) seen so far, and each
// 64-slot chunk is sorted across the lanes (shuffle bitonic network) and
// merged in, most chunks ended by the prefilter against the current k-th key.
// A hub row (above 1024 slots) is dealt out to the 16 waves of a workgroup.
#include "common.h"

#include <limits.h>

namespace bbgr {

constexpr int SLAS_MAX_F = 16;
constexpr int SLAS_MAX_K = 64;

// ---------------------------------------------------------------------------
// Profiles (main.py:727-737)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slas_item_norm_kernel(int n, int F, const float *x,
                                                             long ldx, float *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = x + (long)i * ldx;
  float ss = 0.f;
  for (int f = 0; f < F; ++f) ss = fmaf(p[f], p[f], ss);
  const float den = sqrtf(ss) + 1e-12f;
  for (int f = 0; f < F; ++f) out[(long)i * F + f] = p[f] / den;
}

// One wave per user: lane l sums the slots l, l + 64, ... of the row per
// feature, a fixed xor tree adds the lanes (every lane ends with the same
// bits), then mean and l2n. FM: compile-time feature bound (registers only).
template <int FM>
__global__ __launch_bounds__(256) void slas_user_mu_kernel(int n_users, int F, const int *indptr,
                                                           const int *nbr, const float *item_norm,
                                                           float *user_mu) {
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (u >= n_users) return;   // wave-uniform
  const int rb = indptr[u], re = indptr[u + 1];
  float acc[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) acc[f] = 0.f;
  for (int e = rb + l; e < re; e += 64) {
    const float *p = item_norm + (long)nbr[e] * F;
#pragma unroll
    for (int f = 0; f < FM; ++f)
      if (f < F) acc[f] += p[f];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[f] += __shfl_xor(acc[f], o);
  const float deg = fmaxf((float)(re - rb), 1.f);
  float ss = 0.f;
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    acc[f] = acc[f] / deg;
    ss = fmaf(acc[f], acc[f], ss);
  }
  const float den = sqrtf(ss) + 1e-12f;
#pragma unroll
  for (int f = 0; f < FM; ++f)
    if (l == f && f < F) user_mu[(long)u * F + f] = acc[f] / den;
}

// ---------------------------------------------------------------------------
// Sampler
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool slas_less(float ka, int pa, float kb, int pb) {
  return ka < kb || (ka == kb && pa < pb);
}

// The view filter of one slot (main.py:766-773): early keeps ts < split, late
// ts >= split (a NaN timestamp is in neither, as in numpy).
__device__ __forceinline__ bool slas_eligible(const float *ts, long stride, int view, float split,
                                              int eid) {
  if (view == BBGR_SLAS_VIEW_NONE) return true;
  const float t = ts[(long)eid * stride];
  return view == BBGR_SLAS_VIEW_EARLY ? t < split : t >= split;
}

// One compare-exchange step of a 64-lane bitonic network at distance o: the
// lane keeps the smaller pair when keep_min, else the larger.
__device__ __forceinline__ void slas_cmpx(float &key, int &pos, int o, bool keep_min) {
  const float ok = __shfl_xor(key, o);
  const int op = __shfl_xor(pos, o);
  const bool take = keep_min ? slas_less(ok, op, key, pos) : slas_less(key, pos, ok, op);
  key = take ? ok : key;
  pos = take ? op : pos;
}

// The view-eligible slots among e = rb + start, + step, ... of a row, summed
// over the wave (every lane returns the wave's total).
__device__ __forceinline__ int slas_count(const bbgr_slas_sample_args &A, int rb, int re,
                                          int start, int step) {
  int c = 0;
  for (int e = rb + start; e < re; e += step)
    c += slas_eligible(A.ts, A.ts_stride, A.view, A.split, A.eid[e]) ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
  return c;
}

// m <= k: every eligible slot, in row order (main.py:777-778), -1 behind. One wave.
__device__ __forceinline__ void slas_in_order(const bbgr_slas_sample_args &A, int rb, int re,
                                              int l, int m, int *onbr, int *oeid) {
  int base = 0;
  for (int c = rb; c < re; c += 64) {
    const int e = c + l;
    int eid = 0;
    bool ok = e < re;
    if (ok) {
      eid = A.eid[e];
      ok = slas_eligible(A.ts, A.ts_stride, A.view, A.split, eid);
    }
    const unsigned long long b = __ballot(ok);
    const int pos = base + __popcll(b & ((1ull << l) - 1ull));
    if (ok) {   // pos < m <= k
      onbr[pos] = A.nbr[e];
      oeid[pos] = eid;
    }
    base += __popcll(b);
  }
  if (l >= m && l < A.k) {
    onbr[l] = -1;
    oeid[l] = -1;
  }
}

// A descending list of 64 pairs against the wave's ascending best, lane by
// lane: the 64 smallest of the 128 as a bitonic sequence; a half-cleaner
// cascade sorts it ascending.
__device__ __forceinline__ void slas_merge_desc(float key, int pos, float &bk, int &bp, int l) {
  if (slas_less(key, pos, bk, bp)) {
    bk = key;
    bp = pos;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) slas_cmpx(bk, bp, o, (l & o) == 0);
}

// The 64-slot chunks c0, c0 + cstep, ... of a row merged into the wave's best:
// lane j holds the j-th smallest (key, slot position) so far.
__device__ __forceinline__ void slas_scan(const bbgr_slas_sample_args &A, long row, int rb,
                                          int re, int c0, int cstep, int l, float &bk, int &bp) {
  const int F = A.F, k = A.k;
  const float *rp = A.row_profile + row * F;
  const float up = 1.f + A.upweight;
  const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
  // The slot loads (neighbour, edge id) run one chunk ahead of the gathers that
  // depend on them, so the two are not waited for in a chain.
  const bool view = A.view != BBGR_SLAS_VIEW_NONE;
  bool in_n = c0 + l < re;
  int nb_n = 0, eid_n = 0;
  if (in_n) {
    nb_n = A.nbr[c0 + l];
    if (view) eid_n = A.eid[c0 + l];
  }
  for (int c = c0; c < re; c += cstep) {
    const int e = c + l;
    const bool in = in_n;
    const int nb = nb_n, eid = eid_n;
    const int en = e + cstep;
    in_n = en < re;
    if (in_n) {
      nb_n = A.nbr[en];
      if (view) eid_n = A.eid[en];
    }
    float key = INFINITY;
    int pos = INT_MAX;
    const bool ok = in && slas_eligible(A.ts, A.ts_stride, A.view, A.split, eid);
    if (ok) {
      const float *np = A.nbr_profile + (long)nb * F;
      float dot = 0.f;
      for (int f = 0; f < F; ++f) dot = fmaf(np[f], rp[f], dot);
      float w = expf(A.kappa * dot);
      if (A.label && A.label[nb] >= 0) w *= up;
      w = fminf(fmaxf(w, 1.17549435e-38f), 3.40282347e38f);   // a finite, positive clock rate
      pos = e - rb;
      const u32x4 x = philox4x32_10(u32x4{A.counter, A.stage, (uint32_t)row, (uint32_t)pos}, k0, k1);
      const float u01 = (float)((x.x >> 8) + 1u) * 0x1p-24f;   // (0, 1], exact in fp32
      key = -logf(u01) / w;
    }
    // nothing of this chunk beats the current k-th pair: skip the network
    const float tk = __shfl(bk, k - 1);
    const int tp = __shfl(bp, k - 1);
    if (!__any(ok && slas_less(key, pos, tk, tp))) continue;
    // the chunk in descending order across the lanes
#pragma unroll
    for (int sz = 2; sz <= 64; sz <<= 1)
#pragma unroll
      for (int o = sz >> 1; o >= 1; o >>= 1)
        slas_cmpx(key, pos, o, ((l & o) == 0) != ((l & sz) == 0));
    slas_merge_desc(key, pos, bk, bp, l);
  }
}

// m > k: every one of the k smallest is an eligible slot.
__device__ __forceinline__ void slas_write(const bbgr_slas_sample_args &A, int rb, int l, int bp,
                                           int *onbr, int *oeid) {
  if (l < A.k) {
    const bool have = bp != INT_MAX;
    onbr[l] = have ? A.nbr[rb + bp] : -1;
    oeid[l] = have ? A.eid[rb + bp] : -1;
  }
}

// Rows above this many slots go to the long-row kernel (16 waves per row).
constexpr int SLAS_LONG_ROW = 1024;

__device__ __forceinline__ void slas_row_bounds(const bbgr_slas_sample_args &A, long r, long &row,
                                                int &rb, int &re) {
  row = A.rows[r];
  rb = re = 0;
  if (row >= 0 && row < A.n_rows) {
    rb = A.indptr[row];
    re = A.indptr[row + 1];
  }
}

// One wave per listed row of at most SLAS_LONG_ROW slots.
__global__ __launch_bounds__(256) void slas_sample_kernel(bbgr_slas_sample_args A) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (r >= A.n) return;   // wave-uniform
  long row;
  int rb, re;
  slas_row_bounds(A, r, row, rb, re);
  if (re - rb > SLAS_LONG_ROW) return;   // slas_sample_long_kernel's
  const int k = A.k;
  int *onbr = A.out_nbr + r * k;
  int *oeid = A.out_eid + r * k;
  const int m = A.view != BBGR_SLAS_VIEW_NONE ? slas_count(A, rb, re, l, 64) : re - rb;
  if (l == 0) A.out_count[r] = m < k ? m : k;
  if (m <= k) {
    slas_in_order(A, rb, re, l, m, onbr, oeid);
    return;
  }
  float bk = INFINITY;
  int bp = INT_MAX;
  slas_scan(A, row, rb, re, rb, 64, l, bk, bp);
  slas_write(A, rb, l, bp, onbr, oeid);
}

// The listed rows above SLAS_LONG_ROW slots: a workgroup of 16 waves per row.
// Wave w scans the chunks w, w + 16, ... into its own best 64, the lists meet
// in LDS and wave 0 merges them. The k smallest (key, slot) pairs of a row do
// not depend on how its slots are dealt out, so the picks are those one wave
// would make. (C2's longest item row, 20857 users, alone set the launch's
// time with one wave per row: 0.42 ms against 0.07 ms dealt out)
__global__ __launch_bounds__(1024) void slas_sample_long_kernel(bbgr_slas_sample_args A) {
  __shared__ float s_key[16][64];
  __shared__ int s_pos[16][64];
  __shared__ int s_cnt[16];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int k = A.k;
  for (long r = blockIdx.x; r < A.n; r += gridDim.x) {
    long row;
    int rb, re;
    slas_row_bounds(A, r, row, rb, re);
    if (re - rb <= SLAS_LONG_ROW) continue;   // workgroup-uniform
    int *onbr = A.out_nbr + r * k;
    int *oeid = A.out_eid + r * k;
    int m = re - rb;
    if (A.view != BBGR_SLAS_VIEW_NONE) {
      const int c = slas_count(A, rb, re, threadIdx.x, 1024);
      if (l == 0) s_cnt[w] = c;
      __syncthreads();
      m = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) m += s_cnt[j];
    }
    if (threadIdx.x == 0) A.out_count[r] = m < k ? m : k;
    float bk = INFINITY;
    int bp = INT_MAX;
    if (m > k) slas_scan(A, row, rb, re, rb + 64 * w, 64 * 16, l, bk, bp);
    s_key[w][l] = bk;
    s_pos[w][l] = bp;
    __syncthreads();   // (also: every wave has read s_cnt)
    if (w == 0) {
      if (m <= k) {
        slas_in_order(A, rb, re, l, m, onbr, oeid);
      } else {
        for (int j = 1; j < 16; ++j)   // an ascending list read backwards is descending
          slas_merge_desc(s_key[j][63 - l], s_pos[j][63 - l], bk, bp, l);
        slas_write(A, rb, l, bp, onbr, oeid);
      }
    }
    __syncthreads();   // the lists are free for the next row
  }
}

// mask[ids[j]] = value for the ids >= 0 of a -1-padded int32 list.
__global__ void slas_mark_ids_kernel(long n, const int *ids, unsigned char value,
                                     unsigned char *mask, long n_rows) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int v = ids[j];
  if (v >= 0 && v < n_rows) mask[v] = value;
}

// ---------------------------------------------------------------------------
// Induced edge list (main.py:835-856): count, exclusive scan, fill
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slas_induce_count_kernel(bbgr_slas_induce_args A,
                                                                long long *counts) {
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (j >= A.n_users_listed) return;   // wave-uniform
  const long u = A.users[j];
  int rb = 0, re = 0;
  if (u >= 0 && u < A.n_users) {
    rb = A.indptr[u];
    re = A.indptr[u + 1];
  }
  int c = 0;
  for (int e = rb + l; e < re; e += 64)
    c += (A.item_local[A.nbr[e]] >= 0 &&
          slas_eligible(A.ts, A.ts_stride, A.view, A.split, A.eid[e]))
             ? 1
             : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
  if (l == 0) counts[j] = c;
}

// offs[i] = counts[0] + ... + counts[i-1] for i <= n, *total = offs[n]: one
// workgroup walks the list in tiles of 8192, eight entries per thread (lists
// of 10^5 users: a dozen tiles).
__global__ __launch_bounds__(1024) void slas_scan_kernel(long n, const long long *counts,
                                                         long long *offs, long long *total) {
  __shared__ long long wsum[16];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  long long carry = 0;
  for (long base = 0; base < n; base += 8192) {
    const long i0 = base + 8L * t;
    long long v[8];
    long long s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = i0 + j < n ? counts[i0 + j] : 0;
      s += v[j];
    }
    long long x = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(x, o);
      if (l >= o) x += y;
    }
    if (l == 63) wsum[w] = x;
    __syncthreads();
    long long woff = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long ws = wsum[j];
      woff += j < w ? ws : 0;
      tot += ws;
    }
    long long run = carry + woff + x - s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (i0 + j < n) offs[i0 + j] = run;
      run += v[j];
    }
    carry += tot;
    __syncthreads();
  }
  if (t == 0) {
    offs[n] = carry;
    *total = carry;
  }
}

__global__ __launch_bounds__(256) void slas_induce_fill_kernel(bbgr_slas_induce_args A,
                                                               const long long *offs) {
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (j >= A.n_users_listed) return;   // wave-uniform
  const long u = A.users[j];
  int rb = 0, re = 0;
  if (u >= 0 && u < A.n_users) {
    rb = A.indptr[u];
    re = A.indptr[u + 1];
  }
  long base = (long)offs[j];
  for (int c = rb; c < re; c += 64) {
    const int e = c + l;
    int eid = 0, it = -1;
    if (e < re) {
      eid = A.eid[e];
      if (slas_eligible(A.ts, A.ts_stride, A.view, A.split, eid)) it = A.item_local[A.nbr[e]];
    }
    const bool ok = it >= 0;
    const unsigned long long b = __ballot(ok);
    const long pos = base + __popcll(b & ((1ull << l) - 1ull));
    if (ok && pos < A.capacity) {
      A.out_edges[pos] = j;
      A.out_edges[A.capacity + pos] = it;
      A.out_eid[pos] = eid;
    }
    base += __popcll(b);
  }
}

static bool view_ok(int view) {
  return view == BBGR_SLAS_VIEW_NONE || view == BBGR_SLAS_VIEW_EARLY ||
         view == BBGR_SLAS_VIEW_LATE;
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_slas_profiles(int32_t n_users, int32_t n_items, int32_t F,
                                  const float *item_x, int64_t ldx, const int32_t *indptr_u,
                                  const int32_t *nbr_u, float *item_norm, float *user_mu,
                                  bbgr_stream_t stream) {
  BBGR_REQUIRE(n_users >= 0, "bbgr_slas_profiles: n_users < 0");
  BBGR_REQUIRE(n_items >= 0, "bbgr_slas_profiles: n_items < 0");
  BBGR_REQUIRE(F >= 1 && F <= SLAS_MAX_F, "bbgr_slas_profiles: F not in [1, 16]");
  BBGR_REQUIRE(ldx >= F, "bbgr_slas_profiles: ldx < F");
  if (n_items > 0) {
    BBGR_REQUIRE(item_x, "bbgr_slas_profiles: null item_x");
    BBGR_REQUIRE(item_norm, "bbgr_slas_profiles: null item_norm");
  }
  if (n_users > 0) {
    BBGR_REQUIRE(indptr_u, "bbgr_slas_profiles: null indptr_u");
    BBGR_REQUIRE(nbr_u, "bbgr_slas_profiles: null nbr_u");
    BBGR_REQUIRE(item_norm, "bbgr_slas_profiles: null item_norm");
    BBGR_REQUIRE(user_mu, "bbgr_slas_profiles: null user_mu");
  }
  hipStream_t st = as_stream(stream);
  if (n_items > 0) {
    hipLaunchKernelGGL(slas_item_norm_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256),
                       0, st, n_items, F, item_x, (long)ldx, item_norm);
    BBGR_LAUNCHED("slas_item_norm_kernel");
  }
  if (n_users > 0) {
    const dim3 grid((unsigned)((n_users + 3) / 4));
    if (F <= 2)
      hipLaunchKernelGGL(slas_user_mu_kernel<2>, grid, dim3(256), 0, st, n_users, F, indptr_u,
                         nbr_u, item_norm, user_mu);
    else if (F <= 4)
      hipLaunchKernelGGL(slas_user_mu_kernel<4>, grid, dim3(256), 0, st, n_users, F, indptr_u,
                         nbr_u, item_norm, user_mu);
    else
      hipLaunchKernelGGL(slas_user_mu_kernel<SLAS_MAX_F>, grid, dim3(256), 0, st, n_users, F,
                         indptr_u, nbr_u, item_norm, user_mu);
    BBGR_LAUNCHED("slas_user_mu_kernel");
  }
  return BBGR_OK;
}

extern "C" int bbgr_slas_sample(const bbgr_slas_sample_args *a, bbgr_stream_t stream) {
  BBGR_REQUIRE(a, "bbgr_slas_sample: null args");
  BBGR_REQUIRE(a->n >= 0 && a->n < (int64_t)1 << 31, "bbgr_slas_sample: n out of range");
  BBGR_REQUIRE(a->n_rows >= 0, "bbgr_slas_sample: n_rows < 0");
  BBGR_REQUIRE(a->k >= 1 && a->k <= SLAS_MAX_K, "bbgr_slas_sample: k not in [1, 64]");
  BBGR_REQUIRE(a->F >= 1 && a->F <= SLAS_MAX_F, "bbgr_slas_sample: F not in [1, 16]");
  BBGR_REQUIRE(view_ok(a->view), "bbgr_slas_sample: view not none / early / late");
  BBGR_REQUIRE(a->view == BBGR_SLAS_VIEW_NONE || a->ts,
               "bbgr_slas_sample: a view needs ts (null ts)");
  BBGR_REQUIRE(a->ts == nullptr || a->ts_stride >= 1, "bbgr_slas_sample: ts_stride < 1");
  BBGR_REQUIRE(a->stage < 256u, "bbgr_slas_sample: stage not in [0, 255]");
  if (a->n == 0) return BBGR_OK;
  BBGR_REQUIRE(a->rows, "bbgr_slas_sample: null rows");
  BBGR_REQUIRE(a->indptr, "bbgr_slas_sample: null indptr");
  BBGR_REQUIRE(a->nbr, "bbgr_slas_sample: null nbr");
  BBGR_REQUIRE(a->eid, "bbgr_slas_sample: null eid");
  BBGR_REQUIRE(a->row_profile, "bbgr_slas_sample: null row_profile");
  BBGR_REQUIRE(a->nbr_profile, "bbgr_slas_sample: null nbr_profile");
  BBGR_REQUIRE(a->out_nbr, "bbgr_slas_sample: null out_nbr");
  BBGR_REQUIRE(a->out_eid, "bbgr_slas_sample: null out_eid");
  BBGR_REQUIRE(a->out_count, "bbgr_slas_sample: null out_count");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(slas_sample_kernel, dim3((unsigned)((a->n + 3) / 4)), dim3(256), 0, st, *a);
  BBGR_LAUNCHED("slas_sample_kernel");
  // rows above SLAS_LONG_ROW slots (skipped above): workgroups stride over the list
  hipLaunchKernelGGL(slas_sample_long_kernel, dim3((unsigned)(a->n < 256 ? a->n : 256)),
                     dim3(1024), 0, st, *a);
  BBGR_LAUNCHED("slas_sample_long_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_mark_ids32(int64_t n, const int32_t *ids, uint8_t value, uint8_t *mask,
                               int64_t n_rows, bbgr_stream_t stream) {
  BBGR_REQUIRE(n >= 0, "bbgr_mark_ids32: n < 0");
  BBGR_REQUIRE(n_rows >= 0, "bbgr_mark_ids32: n_rows < 0");
  if (n == 0) return BBGR_OK;
  BBGR_REQUIRE(ids, "bbgr_mark_ids32: null ids");
  BBGR_REQUIRE(mask, "bbgr_mark_ids32: null mask");
  hipLaunchKernelGGL(slas_mark_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), (long)n, ids, value, mask, (long)n_rows);
  BBGR_LAUNCHED("slas_mark_ids_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_slas_induce(const bbgr_slas_induce_args *a, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  BBGR_REQUIRE(a, "bbgr_slas_induce: null args");
  BBGR_REQUIRE(workspace_bytes, "bbgr_slas_induce: null workspace_bytes");
  BBGR_REQUIRE(a->n_users_listed >= 0 && a->n_users_listed < (int64_t)1 << 31,
               "bbgr_slas_induce: n_users_listed out of range");
  BBGR_REQUIRE(a->n_users >= 0, "bbgr_slas_induce: n_users < 0");
  BBGR_REQUIRE(view_ok(a->view), "bbgr_slas_induce: view not none / early / late");
  BBGR_REQUIRE(a->view == BBGR_SLAS_VIEW_NONE || a->ts,
               "bbgr_slas_induce: a view needs ts (null ts)");
  BBGR_REQUIRE(a->ts == nullptr || a->ts_stride >= 1, "bbgr_slas_induce: ts_stride < 1");
  BBGR_REQUIRE(a->capacity >= 0, "bbgr_slas_induce: capacity < 0");
  BBGR_REQUIRE((a->out_edges == nullptr) == (a->out_eid == nullptr),
               "bbgr_slas_induce: out_edges and out_eid must be given together");
  // per listed user (and one more) the count of its induced edges, then their scan
  Carver C;
  const size_t off_counts = C.take_n<long long>((size_t)a->n_users_listed + 1);
  const size_t off_offs = C.take_n<long long>((size_t)a->n_users_listed + 1);
  bool query;
  const int rc = take_workspace("bbgr_slas_induce", C.used, workspace, workspace_bytes, &query);
  if (rc || query || a->n_users_listed == 0) return rc;
  BBGR_REQUIRE(a->users, "bbgr_slas_induce: null users");
  BBGR_REQUIRE(a->item_local, "bbgr_slas_induce: null item_local");
  BBGR_REQUIRE(a->indptr, "bbgr_slas_induce: null indptr");
  BBGR_REQUIRE(a->nbr, "bbgr_slas_induce: null nbr");
  BBGR_REQUIRE(a->eid, "bbgr_slas_induce: null eid");
  hipStream_t st = as_stream(stream);
  long long *counts = ws_at<long long>(workspace, off_counts);
  long long *offs = ws_at<long long>(workspace, off_offs);
  const dim3 grid((unsigned)((a->n_users_listed + 3) / 4));
  if (!a->out_edges) {   // count + scan: the caller sizes the outputs from *count
    BBGR_REQUIRE(a->count, "bbgr_slas_induce: null count");
    hipLaunchKernelGGL(slas_induce_count_kernel, grid, dim3(256), 0, st, *a, counts);
    BBGR_LAUNCHED("slas_induce_count_kernel");
    hipLaunchKernelGGL(slas_scan_kernel, dim3(1), dim3(1024), 0, st, (long)a->n_users_listed,
                       counts, offs, reinterpret_cast<long long *>(a->count));
    BBGR_LAUNCHED("slas_scan_kernel");
    return BBGR_OK;
  }
  if (a->capacity == 0) return BBGR_OK;
  hipLaunchKernelGGL(slas_induce_fill_kernel, grid, dim3(256), 0, st, *a, offs);
  BBGR_LAUNCHED("slas_induce_fill_kernel");
  return BBGR_OK;
}
