// Recommendation lists from bf16 tables, and the pieces that turn them back
// into exact fp32 lists: bbgr_recommend_bf16, bbgr_row_norm_max,
// bbgr_recommend_rescore.
//
// recommend_bf16_kernel is recommend_kernel (recommend.hip) on the bf16 MFMA:
// users on the N side, one per lane r, item tiles staged in LDS, the per-lane
// candidate buffer, flush and sorted register list, the continuation bound,
// the merge (recommend.h) -- with v_mfma_f32_32x32x16_bf16 in place of
// v_mfma_f32_32x32x2_f32: lane half h holds components 16 s + 8 h .. + 7 of
// k-step s, a 32 x 32 score tile takes d / 16 MFMAs instead of d / 2, and the
// user fragment is d / 4 VGPRs instead of d / 2. What the freed registers and
// LDS buy: every width runs 8 waves (256 users) per workgroup, two per SIMD
// (d = 256 ran 128), and d = 128 stages 128-item tiles (was 64).
//
// ---------------------------------------------------------------------------
// The certificate of "bf16_exact" (bbgr_recommend_rescore)
// ---------------------------------------------------------------------------
// u^, i^: the rows rounded to bf16, nearest even: |u^_c - u_c| <= 2^-8 |u_c|
//     (8 significant bits: neighbours of 1 are 2^-7 apart, 1 + 2^-8 a midpoint).
// s^: the bf16 pass's score, sum_c u^_c i^_c accumulated in fp32 (a product of
//     two bf16 has 16 significant bits: exact in fp32).
// s:  the fp32 chain score, fmaf over the components 0, d/2, 1, d/2+1, ...
//
//   |s^ - s| <= eps(d) ||u|| ||i||,   eps(d) = 1.02 * 2^-7 + d * 2^-21.
//
// Operands: |u^_c i^_c - u_c i_c| <= (2 * 2^-8 + 2^-16) |u_c| |i_c|, and
// sum_c |u_c| |i_c| <= ||u|| ||i|| (Cauchy-Schwarz): 2^-7 + 2^-16 < 1.02 * 2^-7
// (the remaining 2^-13 absorbs the second-order terms below). Rows of one sign
// on rounding midpoints reach 2^-7 (tests/test_recommend_bf16_bound.py).
// Accumulation: the fp32 chain makes d roundings of at most 2^-24 (half an
// ulp) of a partial sum bounded by sum |u_c| |i_c|, the MFMA's d additions are
// allowed a whole ulp, 2^-23, each: together 3 d 2^-24 sum |u_c| |i_c| =
// 0.375 d 2^-21 ||u|| ||i||, under d * 2^-21 with a factor > 2 to spare.
// Underflow: a subnormal operand is rounded (or flushed by the matrix pipe)
// with an absolute error of at most 2^-126, which adds at most 2^-126 * 1.01 *
// sum_c (|u_c| + |i_c|) <= 2^-121 (||u|| + ||i||) (sqrt(d) <= 16); subnormal
// partial sums, rounded or flushed, add at most 2 d 2^-126 <= 2^-117 per chain.
//
// The bf16 pass returns K' candidates per user; t^ is its K'-th score. Every
// eligible item outside the candidates has s^ <= t^, so s <= t^ + E_u with
//   E_u = eps(d) ||u|| N_max + 2^-121 (||u|| + N_max) + 2^-116,
//   N_max >= max_i ||i||.
// A user is certified when its candidate row is not full (fewer than K'
// eligible items exist: the candidates are all of them) or the k-th best fp32
// chain score among the candidates is STRICTLY greater than t^ + E_u: then no
// outside item can reach position k or tie with it, so tie groups are safe.
// The comparison is made in double (t^ + E_u is not rounded down to t^ unless
// E_u is below half a double ulp of t^, and then s_k > t^ already implies it).
// ||u|| and N_max are upper bounds: fp32 sums of squares in a fixed order of
// at most 20 roundings (relative error <= 20 * 2^-24 of the sum, 10 * 2^-24 of
// the root), the root (<= 2^-23), times 1 + 2^-20 in one fma with the absolute
// 2^-58 that covers squares lost to underflow (<= 256 * 2^-126 of the sum):
// (1 - 13 * 2^-24)(1 + 2^-20) > 1. NaN or infinite norms, norms above 2^60
// (beyond them a bf16 rounding or a score could overflow where fp32 does not)
// and non-finite fp32 scores among the candidates leave the user uncertified.
#include "recommend.h"

namespace bbgr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 256 users per workgroup at every width; items per LDS tile; LDS: 2 tiles of
// TILE x (D + 8) bf16 + CB x THREADS float2 (86, 116 and 114 KB).
template <int D> struct RecBf16Shape {
  static constexpr int THREADS = 512;
  static constexpr int USERS = THREADS / 2;
  static constexpr int TILE = D == 256 ? 64 : 128;
  static constexpr int CB = 12;
  static constexpr int LDT = D + 8;   // padded LDS row, bf16 elements: rows 16 bytes apart
                                      // mod 128, so a wave's ds_read_b128 is conflict-free
  static constexpr size_t lds_bytes() {
    return sizeof(uint16_t) * 2 * TILE * LDT + sizeof(float2) * CB * THREADS;
  }
};

// recommend_kernel's structure, statement for statement, but for the tile
// staging (16-byte chunks of 8 bf16) and the scoring chain.
template <int D, int KM>
__global__ __launch_bounds__(RecBf16Shape<D>::THREADS) void recommend_bf16_kernel(RecParams P) {
  constexpr int THREADS = RecBf16Shape<D>::THREADS;
  constexpr int USERS = RecBf16Shape<D>::USERS;
  constexpr int TILE = RecBf16Shape<D>::TILE;
  constexpr int CB = RecBf16Shape<D>::CB;
  constexpr int LDT = RecBf16Shape<D>::LDT;
  constexpr int M = TILE / 32;        // 32-item sub-tiles (one accumulator each)
  constexpr int S = D / 16;           // k-steps (one MFMA per sub-tile each)
  constexpr int C8 = D / 8;           // 16-byte chunks per row
  constexpr int F8 = TILE * C8 / THREADS;   // chunks per thread per tile
  static_assert(M >= 2 && M % 2 == 0 && TILE * C8 % THREADS == 0 && LDT % 8 == 0, "tile shape");
  extern __shared__ uint4 smem16[];
  uint16_t *tile = reinterpret_cast<uint16_t *>(smem16);                  // [2][TILE][LDT]
  float2 *cbuf = reinterpret_cast<float2 *>(tile + 2 * TILE * LDT);       // [CB][THREADS]
  const uint16_t *uf = static_cast<const uint16_t *>(P.uf);
  const uint16_t *itf = static_cast<const uint16_t *>(P.itf);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  const long b = (long)blockIdx.x * USERS + w * 32 + r;
  const bool valid = b < P.n_users;
  const long u = valid ? P.users[b] : 0;
  const int split = blockIdx.y;
  const int item_lo = split * P.split_items;
  const int item_hi = min(P.n_items, item_lo + P.split_items);
  // user fragment: components 16 s + 8 h + j of user u, j = 0..7, per k-step s
  bf16x8 ub[S];
  {
    const uint4 *pu = reinterpret_cast<const uint4 *>(uf + u * P.lduf + 8 * h);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const uint4 v = valid ? pu[2 * s] : make_uint4(0u, 0u, 0u, 0u);
      ub[s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  // The pair this pass continues after: a candidate is admitted only if it
  // sorts strictly after (ps, pi). The first pass admits every finite score.
  float ps = INFINITY;
  int pi = -1;
  bool live = valid;
  if (valid && P.cont) {
    ps = P.bound_score[b];
    pi = P.bound_item[b];
    live = pi != INT_MAX;   // the previous pass ran out of items: nothing is left
  }
  // exclusion row pointer (monotone; starts at the first excluded item >= item_lo)
  int tp = 0, tend = 0, nt = INT_MAX;
  if (live && P.ex_indptr) {
    const int rb = P.ex_indptr[u], re = P.ex_indptr[u + 1];
    tp = rb + lower_bound_i32(P.ex_indices + rb, re - rb, item_lo);
    tend = re;
    nt = tp < tend ? P.ex_indices[tp] : INT_MAX;
  }
  float tv[KM];
  int ti[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    tv[j] = -INFINITY;
    ti[j] = INT_MAX;
  }
  int cnt = 0;
  // (+inf for a lane without a live user: nothing ever passes its threshold)
  float thr = live ? -INFINITY : INFINITY;
  auto flush = [&]() {
    for (int j = 0; j < cnt; ++j) {
      const float2 c = cbuf[j * THREADS + threadIdx.x];
      const float sc = c.x;
      const int it = __float_as_int(c.y);
      if (sc > tv[KM - 1]) {
        while (nt < it) nt = ++tp < tend ? P.ex_indices[tp] : INT_MAX;
        const bool drop = nt == it || (P.item_mask && P.item_mask[it] == 0);
        if (!drop) topk_insert<KM>(tv, ti, sc, it);
      }
    }
    cnt = 0;
    thr = live ? tv[KM - 1] : INFINITY;
  };
  const int n_tiles = item_hi > item_lo ? (item_hi - item_lo + TILE - 1) / TILE : 0;
  uint4 stage[F8];
  auto load_tile = [&](int t) {
    const int i0 = item_lo + t * TILE;
#pragma unroll
    for (int j = 0; j < F8; ++j) {
      const int f = threadIdx.x + THREADS * j;
      const int row = f / C8, c8 = f % C8;
      const int it = i0 + row;
      stage[j] = it < item_hi ? reinterpret_cast<const uint4 *>(itf + (long)it * P.ldif)[c8]
                              : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_tile = [&](int buf) {
    uint16_t *T = tile + buf * TILE * LDT;
#pragma unroll
    for (int j = 0; j < F8; ++j) {
      const int f = threadIdx.x + THREADS * j;
      const int row = f / C8, c8 = f % C8;
      *reinterpret_cast<uint4 *>(T + row * LDT + 8 * c8) = stage[j];
    }
  };
  // Scores of sub-tiles [lo, hi) of tile T: per sub-tile one chain of S MFMAs.
  // Sub-tiles [plo, phi) (already scored) have their maxima folded into mxp
  // between the MFMAs, 16 / S elements per step.
  f32x16 acc[M];
  float mxp[M];
  auto score_rows = [&](const uint16_t *T, int lo, int hi, int plo, int phi) {
#pragma unroll
    for (int m = lo; m < hi; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
#pragma unroll
    for (int m = plo; m < phi; ++m) mxp[m] = acc[m][0];
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int m = plo; m < phi; ++m)
#pragma unroll
        for (int e = s * 16 / S; e < (s + 1) * 16 / S; ++e)
          if (e > 0) mxp[m] = fmaxf(mxp[m], acc[m][e]);
      bf16x8 a[M];
#pragma unroll
      for (int m = lo; m < hi; ++m)
        a[m] = *reinterpret_cast<const bf16x8 *>(T + (m * 32 + r) * LDT + 16 * s + 8 * h);
#pragma unroll
      for (int m = lo; m < hi; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], ub[s], acc[m], 0, 0, 0);
    }
  };
  // Sub-tile m's scores against the threshold; acc[m][e] = score of user b,
  // item i0 + 32m + (e&3) + 8(e>>2) + 4h.
  auto scan = [&](int m, int i0) {
    if (mxp[m] > thr) {
      unsigned pass = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        pass |= (acc[m][e] > thr && acc[m][e] <= ps ? 1u : 0u) << e;
      while (pass) {
        const int e = __builtin_ctz(pass);
        pass &= pass - 1;
        float sc = acc[m][0];
#pragma unroll
        for (int e2 = 1; e2 < 16; ++e2) sc = e2 == e ? acc[m][e2] : sc;
        const int it = i0 + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (it < item_hi && (sc < ps || it > pi)) {
          if (cnt == CB) flush();      // this lane only (early tiles: all lanes together)
          cbuf[cnt * THREADS + threadIdx.x] = make_float2(sc, __int_as_float(it));
          ++cnt;
        }
      }
    }
    if (__any(cnt > CB - 4)) flush();   // batch the insertions across lanes
  };
  if (n_tiles > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  // Software pipeline, as in recommend_kernel: the second half of tile t-1's
  // sub-tiles is checked while the first half of tile t is on the MFMA pipe.
  constexpr int M2 = M / 2;
#pragma unroll
  for (int m = M2; m < M; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = -INFINITY;
  int i_prev = item_lo;
  for (int t = 0; t < n_tiles; ++t) {
    if (t + 1 < n_tiles) load_tile(t + 1);
    const uint16_t *T = tile + (t & 1) * TILE * LDT;
    const int i0 = item_lo + t * TILE;
    score_rows(T, 0, M2, M2, M);
#pragma unroll
    for (int m = M2; m < M; ++m) scan(m, i_prev);
    score_rows(T, M2, M, 0, M2);
#pragma unroll
    for (int m = 0; m < M2; ++m) scan(m, i0);
    i_prev = i0;
    if (t + 1 < n_tiles) store_tile((t + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int m = M2; m < M; ++m) {
    mxp[m] = acc[m][0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mxp[m] = fmaxf(mxp[m], acc[m][e]);
    scan(m, i_prev);
  }
  flush();
  if (valid) {
    const long o = ((b * P.n_splits + split) * 2 + h) * KM;
#pragma unroll
    for (int j = 0; j < KM; ++j) {
      P.list_score[o + j] = tv[j];
      P.list_item[o + j] = ti[j];
    }
  }
}

// ---------------------------------------------------------------------------
// Norm bounds
// ---------------------------------------------------------------------------
constexpr float NORM_INFLATE = 1.0f + 0x1p-20f;
constexpr float NORM_FLOOR = 0x1p-58f;
constexpr float NORM_LIMIT = 0x1p60f;

// The sum of squares of a d-wide row (d % 4 == 0, d <= 256) over a 16-lane
// group: lane l16 takes the float4 columns l16, l16 + 16, ... in order (at most
// 16 roundings), then a butterfly over the group (4 more). Every lane of the
// group calls it and gets the sum.
__device__ __forceinline__ float row_sumsq16(const float *row, int d, int l16) {
  float q = 0.f;
  for (int c = l16; c < d / 4; c += 16) {
    const float4 v = reinterpret_cast<const float4 *>(row)[c];
    q = fmaf(v.x, v.x, q);
    q = fmaf(v.y, v.y, q);
    q = fmaf(v.z, v.z, q);
    q = fmaf(v.w, v.w, q);
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) q += __shfl_xor(q, o);
  return q;
}

// An upper bound of the norm from row_sumsq16's sum (the header of this file).
__device__ __forceinline__ float norm_upper(float sumsq) {
  return fmaf(sqrtf(sumsq), NORM_INFLATE, NORM_FLOOR);
}

// out[0] = max over rows of norm_upper, as the integer max of the bit patterns
// (non-negative floats order as their bits; a NaN sorts above +inf and stays).
__global__ __launch_bounds__(256) void row_norm_max_kernel(long n_rows, int d, const float *src,
                                                          long ld, unsigned *out) {
  __shared__ unsigned part[4];
  const int l16 = threadIdx.x & 15;
  const long groups = (long)gridDim.x * 16;
  unsigned best = 0;
  for (long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4); row < n_rows; row += groups) {
    const float v = norm_upper(row_sumsq16(src + row * ld, d, l16));
    best = max(best, __float_as_uint(v) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) best = max(best, (unsigned)__shfl_xor((int)best, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(out, max(max(part[0], part[1]), max(part[2], part[3])));
}

// ---------------------------------------------------------------------------
// Rescoring
// ---------------------------------------------------------------------------
struct RescoreParams {
  const long *users;
  const float *uf, *itf;
  long lduf, ldif;
  int n_items, k, k_pre;
  const int *cand;
  const float *cand_score;
  const float *n_max;
  int *topk;
  float *topk_score;
  unsigned char *certified;
};

// One workgroup per user, one lane per candidate: the lane runs the serial fma
// chain of recommend_kernel (item component times user component, components
// 0, d/2, 1, d/2+1, ...), so the score has that kernel's bits. The candidates
// are ranked by counting ((score desc, item asc), distinct items: distinct
// ranks); the first k are written and lane 0 decides the certificate.
template <int D>
__global__ __launch_bounds__(REC_MAX_K) void recommend_rescore_kernel(RescoreParams P) {
  constexpr int H = D / 2;
  __shared__ float4 us4[D / 4];
  __shared__ float ss[REC_MAX_K];
  __shared__ int si[REC_MAX_K];
  __shared__ float norm_u, s_k;
  __shared__ int bad;
  const long b = blockIdx.x;
  const int j = threadIdx.x;
  const long u = P.users[b];
  const float *urow = P.uf + u * P.lduf;
  if (j < D / 4) us4[j] = reinterpret_cast<const float4 *>(urow)[j];
  if (j < 64) {   // one whole wave: the butterfly reads inside each 16-lane group
    const float q = row_sumsq16(urow, D, j & 15);
    if (j == 0) {
      norm_u = norm_upper(q);
      bad = 0;
      s_k = -INFINITY;
    }
  }
  __syncthreads();
  const int it = j < P.k_pre ? P.cand[b * P.k_pre + j] : -1;
  const bool have = it >= 0 && it < P.n_items;
  float sc = -INFINITY;
  if (have) {
    const float4 *pi = reinterpret_cast<const float4 *>(P.itf + (long)it * P.ldif);
    float acc = 0.f;
#pragma unroll 4
    for (int s4 = 0; s4 < H / 4; ++s4) {
      const float4 a = pi[s4], c = pi[H / 4 + s4];
      const float4 x = us4[s4], y = us4[H / 4 + s4];
      acc = fmaf(a.x, x.x, acc);
      acc = fmaf(c.x, y.x, acc);
      acc = fmaf(a.y, x.y, acc);
      acc = fmaf(c.y, y.y, acc);
      acc = fmaf(a.z, x.z, acc);
      acc = fmaf(c.z, y.z, acc);
      acc = fmaf(a.w, x.w, acc);
      acc = fmaf(c.w, y.w, acc);
    }
    if (!isfinite(acc)) bad = 1;          // (a plain store: every writer writes 1)
    sc = acc == acc ? acc : -INFINITY;    // a NaN ranks last; its user is not certified
  }
  const int key = have ? it : INT_MAX;
  ss[j] = sc;
  si[j] = key;
  __syncthreads();
  int rank = 0;
  for (int i = 0; i < REC_MAX_K; ++i) {
    const float os = ss[i];
    const int oi = si[i];
    rank += os > sc || (os == sc && (oi < key || (oi == key && i < j)));
  }
  if (rank < P.k) {
    const long o = b * P.k + rank;
    P.topk[o] = have ? it : -1;
    if (P.topk_score) P.topk_score[o] = have ? sc : -INFINITY;
    if (rank == P.k - 1) s_k = sc;
  }
  __syncthreads();
  if (j == 0) {
    const long last = b * P.k_pre + P.k_pre - 1;
    const bool full = P.cand[last] >= 0;
    const float n_max = *P.n_max;
    bool ok = !bad && norm_u <= NORM_LIMIT && n_max <= NORM_LIMIT;   // (a NaN compares false)
    if (ok && full) {
      const double eps = 1.02 * 0x1p-7 + D * 0x1p-21;
      const double nu = norm_u, nm = n_max;
      const double e_u = eps * nu * nm + 0x1p-121 * (nu + nm) + 0x1p-116;
      ok = (double)s_k > (double)P.cand_score[last] + e_u;
    }
    P.certified[b] = ok ? 1 : 0;
  }
}

template <int D, int KM>
static int launch_recommend_bf16(const RecParams &P, hipStream_t st) {
  const size_t lds = RecBf16Shape<D>::lds_bytes();
  BBGR_HIP(hipFuncSetAttribute((const void *)recommend_bf16_kernel<D, KM>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  constexpr int USERS = RecBf16Shape<D>::USERS;
  const dim3 grid((unsigned)((P.n_users + USERS - 1) / USERS), (unsigned)P.n_splits);
  hipLaunchKernelGGL((recommend_bf16_kernel<D, KM>), grid, dim3(RecBf16Shape<D>::THREADS), lds,
                     st, P);
  BBGR_LAUNCHED("recommend_bf16_kernel");
  return BBGR_OK;
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_recommend_bf16(const bbgr_recommend_bf16_args *a, void *workspace,
                                   size_t *workspace_bytes, bbgr_stream_t stream) {
  if (const int rc = rec_check_args("bbgr_recommend_bf16", a, workspace_bytes, 8)) return rc;
  const int d = a->d;
  return rec_run("bbgr_recommend_bf16", a, workspace, workspace_bytes, RecBf16Shape<64>::USERS,
                 stream, [d](const RecParams &P, int km, hipStream_t st) {
                   return for_wide_width(d, [&](auto W) {
                     constexpr int D = decltype(W)::value;
                     return km == 16 ? launch_recommend_bf16<D, 16>(P, st)
                                     : launch_recommend_bf16<D, 24>(P, st);
                   });
                 });
}

extern "C" int bbgr_row_norm_max(int64_t n_rows, int32_t d, const float *src, int64_t ld,
                                 float *out, bbgr_stream_t stream) {
  BBGR_REQUIRE(n_rows >= 0, "bbgr_row_norm_max: n_rows < 0");
  BBGR_REQUIRE(d >= 4 && d <= 256 && (d & 3) == 0,
               "bbgr_row_norm_max: d must be a multiple of 4 in [4, 256]");
  BBGR_REQUIRE(out, "bbgr_row_norm_max: null out");
  BBGR_REQUIRE(n_rows == 0 || src, "bbgr_row_norm_max: null src");
  BBGR_REQUIRE(n_rows == 0 || ld_ok(src, ld, d),
               "bbgr_row_norm_max: src must be 16-byte aligned with ld >= d, ld % 4 == 0");
  hipStream_t st = as_stream(stream);
  BBGR_HIP(hipMemsetAsync(out, 0, sizeof(float), st));
  if (n_rows == 0) return BBGR_OK;
  const long want = (n_rows + 15) / 16;
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(row_norm_max_kernel, dim3(grid), dim3(256), 0, st, (long)n_rows, (int)d, src,
                     (long)ld, reinterpret_cast<unsigned *>(out));
  BBGR_LAUNCHED("row_norm_max_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_recommend_rescore(const bbgr_recommend_rescore_args *a,
                                      bbgr_stream_t stream) {
  const char *who = "bbgr_recommend_rescore";
  BBGR_REQUIRE_IN(who, a, "null args");
  BBGR_REQUIRE_IN(who, a->n_users >= 0, "n_users < 0");
  BBGR_REQUIRE_IN(who, a->k >= 1 && a->k <= REC_MAX_K, "k not in [1, 128]");
  BBGR_REQUIRE_IN(who, a->k_pre >= a->k && a->k_pre <= REC_MAX_K, "k_pre not in [k, 128]");
  BBGR_REQUIRE_IN(who, a->n_items > 0, "n_items <= 0");
  BBGR_REQUIRE_IN(who, a->n_user_rows > 0, "n_user_rows <= 0");
  if (a->n_users > 0) {
    BBGR_REQUIRE_IN(who, a->users, "null users");
    BBGR_REQUIRE_IN(who, a->uf, "null uf");
    BBGR_REQUIRE_IN(who, a->itf, "null itf");
    BBGR_REQUIRE_IN(who, a->cand, "null cand");
    BBGR_REQUIRE_IN(who, a->cand_score, "null cand_score");
    BBGR_REQUIRE_IN(who, a->n_max, "null n_max");
    BBGR_REQUIRE_IN(who, a->topk, "null topk");
    BBGR_REQUIRE_IN(who, a->certified, "null certified");
  }
  BBGR_REQUIRE_IN(who, aligned16(a->uf) && (a->lduf & 3) == 0,
                  "uf must be 16-byte aligned, lduf % 4 == 0");
  BBGR_REQUIRE_IN(who, aligned16(a->itf) && (a->ldif & 3) == 0,
                  "itf must be 16-byte aligned, ldif % 4 == 0");
  const int d = a->d;
  if (d != 64 && d != 128 && d != 256) return unsupported_width(who, d, true);
  BBGR_REQUIRE_IN(who, a->n_users == 0 || (a->lduf >= d && a->ldif >= d), "lduf / ldif < d");
  BBGR_REQUIRE_IN(who, a->n_users <= 0x7fffffffL, "n_users too large for one launch");
  if (a->n_users == 0) return BBGR_OK;
  RescoreParams P;
  P.users = (const long *)a->users;
  P.uf = a->uf;
  P.itf = a->itf;
  P.lduf = a->lduf;
  P.ldif = a->ldif;
  P.n_items = a->n_items;
  P.k = a->k;
  P.k_pre = a->k_pre;
  P.cand = a->cand;
  P.cand_score = a->cand_score;
  P.n_max = a->n_max;
  P.topk = a->topk;
  P.topk_score = a->topk_score;
  P.certified = a->certified;
  hipStream_t st = as_stream(stream);
  return for_wide_width(d, [&](auto W) {
    hipLaunchKernelGGL(recommend_rescore_kernel<decltype(W)::value>, dim3((unsigned)a->n_users),
                       dim3(REC_MAX_K), 0, st, P);
    BBGR_LAUNCHED("recommend_rescore_kernel");
    return (int)BBGR_OK;
  });
}
