// Recommendation lists: the top-k items of a caller's users, k <= 128, at
// d in {64, 128, 256}.
//
// The scoring chain is eval_full_kernel's (eval.hip): fp32 MFMA
// (v_mfma_f32_32x32x2_f32) over LDS-staged item tiles, lane half h holding the
// components h*d/2 + s, so every score is one fp32 fma chain over the
// components 0, d/2, 1, d/2+1, ... Each lane keeps a sorted register list of
// depth KM (16 or 24) of the items it owns, (score desc, item asc), gated by a
// per-sub-tile max; a merge kernel combines the per-lane lists of a user.
//
// What differs from the evaluation kernel:
//  - excluded items (a nullable CSR over user ids, rows sorted ascending,
//    duplicates allowed) and items outside a nullable byte mask are DROPPED on
//    the insertion path, not scored -1e9: a list holds eligible items only and
//    ends in -1 / -inf where fewer than k exist;
//  - k > KM runs continuation passes: pass p admits only the candidates
//    strictly after the user's last (score, item) pair of pass p-1 in the list
//    order, read from the merge's per-user bound, so ceil(k / KM) passes give
//    the exact top-k, tie groups that straddle a pass boundary included;
//  - d = 256: 128 user components per lane do not fit beside the lists at two
//    waves per SIMD, so that form runs 4 waves (128 users) per workgroup, one
//    per SIMD, with the whole unified register file.
#include "recommend.h"

namespace bbgr {

// Threads / users per workgroup, items per LDS tile and per-lane candidate
// buffer depth, per embedding dim (LDS: 2 tiles of TILE x (D+4) floats + CB x
// THREADS float2 <= 160 KB).
template <int D> struct RecShape {
  static constexpr int THREADS = D == 256 ? 256 : 512;
  static constexpr int USERS = THREADS / 2;
  static constexpr int TILE = D == 64 ? 128 : 64;
  static constexpr int CB = 12;
  static constexpr size_t lds_bytes() {
    return sizeof(float) * 2 * TILE * (D + 4) + sizeof(float2) * CB * THREADS;
  }
};

template <int D, int KM>
__global__ __launch_bounds__(RecShape<D>::THREADS) void recommend_kernel(RecParams P) {
  constexpr int THREADS = RecShape<D>::THREADS;
  constexpr int USERS = RecShape<D>::USERS;
  constexpr int TILE = RecShape<D>::TILE;
  constexpr int CB = RecShape<D>::CB;
  constexpr int M = TILE / 32;        // 32-item sub-tiles (one accumulator each)
  constexpr int LDT = D + 4;          // padded LDS row (conflict-free b128 reads)
  constexpr int H = D / 2;            // components per lane half
  constexpr int S = H / 4;            // component steps (4 MFMAs per sub-tile each)
  constexpr int F4 = TILE * D / 4 / THREADS;   // float4 per thread per tile
  static_assert(M >= 2 && M % 2 == 0 && TILE * D / 4 % THREADS == 0, "tile shape");
  extern __shared__ float smem[];
  float *tile = smem;                                                  // [2][TILE][LDT]
  float2 *cbuf = reinterpret_cast<float2 *>(smem + 2 * TILE * LDT);   // [CB][THREADS]
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  const long b = (long)blockIdx.x * USERS + w * 32 + r;
  const bool valid = b < P.n_users;
  const long u = valid ? P.users[b] : 0;
  const int split = blockIdx.y;
  const int item_lo = split * P.split_items;
  const int item_hi = min(P.n_items, item_lo + P.split_items);
  // user fragment: component h*H + s of user u, for s = 0..H-1
  float ub[H];
  {
    const float4 *pu = reinterpret_cast<const float4 *>(static_cast<const float *>(P.uf) + u * P.lduf + h * H);
#pragma unroll
    for (int s = 0; s < H / 4; ++s) {
      const float4 v = valid ? pu[s] : make_float4(0.f, 0.f, 0.f, 0.f);
      ub[4 * s] = v.x;
      ub[4 * s + 1] = v.y;
      ub[4 * s + 2] = v.z;
      ub[4 * s + 3] = v.w;
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
  // Candidates whose score beats the (possibly stale) threshold are appended
  // to the lane's LDS buffer in ascending item order; a flush inserts every
  // lane's buffer at once. Exclusion and the item mask are tested here only,
  // for candidates that still beat the list's last entry.
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
  float4 stage[F4];
  auto load_tile = [&](int t) {
    const int i0 = item_lo + t * TILE;
#pragma unroll
    for (int j = 0; j < F4; ++j) {
      const int f = threadIdx.x + THREADS * j;
      const int row = f / (D / 4), c4 = f % (D / 4);
      const int it = i0 + row;
      stage[j] = it < item_hi ? reinterpret_cast<const float4 *>(static_cast<const float *>(P.itf) + (long)it * P.ldif)[c4]
                              : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_tile = [&](int buf) {
    float *T = tile + buf * TILE * LDT;
#pragma unroll
    for (int j = 0; j < F4; ++j) {
      const int f = threadIdx.x + THREADS * j;
      const int row = f / (D / 4), c4 = f % (D / 4);
      *reinterpret_cast<float4 *>(T + row * LDT + 4 * c4) = stage[j];
    }
  };
  // Scores of sub-tiles [lo, hi) of tile T: per sub-tile one chain of H MFMAs
  // over the components in order. Sub-tiles [plo, phi) (already scored) have
  // their maxima folded into mxp between the MFMAs, 16 / S elements per step
  // (one every other step at d = 256), so the check's VALU work issues while
  // the matrix pipe is busy.
  f32x16 acc[M];
  float mxp[M];
  auto score_rows = [&](const float *T, int lo, int hi, int plo, int phi) {
#pragma unroll
    for (int m = lo; m < hi; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
#pragma unroll
    for (int m = plo; m < phi; ++m) mxp[m] = acc[m][0];
#pragma unroll
    for (int s4 = 0; s4 < S; ++s4) {
#pragma unroll
      for (int m = plo; m < phi; ++m)
#pragma unroll
        for (int e = s4 * 16 / S; e < (s4 + 1) * 16 / S; ++e)
          if (e > 0) mxp[m] = fmaxf(mxp[m], acc[m][e]);
      float4 a[M];
#pragma unroll
      for (int m = lo; m < hi; ++m)
        a[m] = *reinterpret_cast<const float4 *>(T + (m * 32 + r) * LDT + h * H + 4 * s4);
      // independent accumulators back to back
#pragma unroll
      for (int m = lo; m < hi; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].x, ub[4 * s4 + 0], acc[m], 0, 0, 0);
#pragma unroll
      for (int m = lo; m < hi; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].y, ub[4 * s4 + 1], acc[m], 0, 0, 0);
#pragma unroll
      for (int m = lo; m < hi; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].z, ub[4 * s4 + 2], acc[m], 0, 0, 0);
#pragma unroll
      for (int m = lo; m < hi; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].w, ub[4 * s4 + 3], acc[m], 0, 0, 0);
    }
  };
  // Sub-tile m's scores against the threshold; acc[m][e] = score of user b,
  // item i0 + 32m + (e&3) + 8(e>>2) + 4h. The sub-tile max gates the whole
  // check; the continuation bound is tested for the scores that pass it.
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
  // Software pipeline: the second half of tile t-1's sub-tiles is checked
  // while the first half of tile t is on the MFMA pipe, the first half of
  // tile t while its second half is. Candidates still reach each lane's
  // buffer in ascending item order. (Before the first tile the pending half
  // holds -inf scores: nothing passes.)
  constexpr int M2 = M / 2;
#pragma unroll
  for (int m = M2; m < M; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = -INFINITY;
  int i_prev = item_lo;
  for (int t = 0; t < n_tiles; ++t) {
    if (t + 1 < n_tiles) load_tile(t + 1);
    const float *T = tile + (t & 1) * TILE * LDT;
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
// Host side
// ---------------------------------------------------------------------------
static int rec_users(int d) { return d == 256 ? RecShape<256>::USERS : RecShape<64>::USERS; }

template <int D, int KM>
static int launch_recommend(const RecParams &P, hipStream_t st) {
  const size_t lds = RecShape<D>::lds_bytes();
  BBGR_HIP(hipFuncSetAttribute((const void *)recommend_kernel<D, KM>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  constexpr int USERS = RecShape<D>::USERS;
  const dim3 grid((unsigned)((P.n_users + USERS - 1) / USERS), (unsigned)P.n_splits);
  hipLaunchKernelGGL((recommend_kernel<D, KM>), grid, dim3(RecShape<D>::THREADS), lds, st, P);
  BBGR_LAUNCHED("recommend_kernel");
  return BBGR_OK;
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_recommend(const bbgr_recommend_args *a, void *workspace,
                              size_t *workspace_bytes, bbgr_stream_t stream) {
  if (const int rc = rec_check_args("bbgr_recommend", a, workspace_bytes, 4)) return rc;
  const int d = a->d;
  return rec_run("bbgr_recommend", a, workspace, workspace_bytes, rec_users(d), stream,
                 [d](const RecParams &P, int km, hipStream_t st) {
                   switch (d * 100 + km) {
                     case 6416: return launch_recommend<64, 16>(P, st);
                     case 6424: return launch_recommend<64, 24>(P, st);
                     case 12816: return launch_recommend<128, 16>(P, st);
                     case 12824: return launch_recommend<128, 24>(P, st);
                     case 25616: return launch_recommend<256, 16>(P, st);
                     default: return launch_recommend<256, 24>(P, st);
                   }
                 });
}
