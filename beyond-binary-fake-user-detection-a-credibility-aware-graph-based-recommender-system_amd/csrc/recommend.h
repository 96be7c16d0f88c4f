// What the two recommendation scorers share (recommend.hip's fp32
// recommend_kernel, recommend_bf16.hip's recommend_bf16_kernel): the launch
// parameters, the per-user merge of the per-lane lists, the workspace layout
// and the argument checks of the two entry points.
#pragma once

#include "topk.h"

namespace bbgr {

constexpr int REC_MAX_K = 128;

struct RecParams {
  long n_users;               // users in this launch
  const long *users;
  const int *ex_indptr, *ex_indices;   // nullable together
  const unsigned char *item_mask;      // nullable, [n_items], nonzero = eligible
  const void *uf, *itf;       // float tables (recommend_kernel) or bf16 (recommend_bf16_kernel)
  long lduf, ldif;            // in elements
  int n_items;
  int split_items;            // items per split (multiple of FULL_TILE)
  int n_splits;
  int cont;                   // 0 first pass, 1 continuation pass (reads the bound)
  float *list_score;          // [n_users][n_splits][2][KM]
  int *list_item;
  float *bound_score;         // [n_users]: the last pair the previous pass emitted
  int *bound_item;            //            (INT_MAX: the user has no items left)
};

// Per user (one wave): merge the 2 * n_splits sorted lists into the next
// `n` (<= KM) entries of the user's list, positions [pos0, pos0 + n) of k, and
// leave the last merged pair as the next pass's bound.
template <int KM>
__global__ __launch_bounds__(256) void recommend_merge_kernel(RecParams P, long b0, int k,
                                                              int pos0, int n, int *topk,
                                                              float *topk_score) {
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (b >= P.n_users) return;   // wave-uniform
  const int L = 2 * P.n_splits;
  const long base = b * L * KM;
  int p = 0;
  float hs = -INFINITY;
  int hi = INT_MAX;
  if (l < L) {
    hs = P.list_score[base + l * KM];
    hi = P.list_item[base + l * KM];
  }
  for (int j = 0; j < n; ++j) {
    float bs = hs;
    int bi = hi, bl = l;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float os = __shfl_xor(bs, o);
      const int oi = __shfl_xor(bi, o);
      const int ol = __shfl_xor(bl, o);
      const bool take = os > bs || (os == bs && (oi < bi || (oi == bi && ol < bl)));
      bs = take ? os : bs;
      bi = take ? oi : bi;
      bl = take ? ol : bl;
    }
    if (l == 0) {
      const long o = (b0 + b) * k + pos0 + j;
      topk[o] = bi == INT_MAX ? -1 : bi;
      if (topk_score) topk_score[o] = bi == INT_MAX ? -INFINITY : bs;
      if (j == n - 1) {
        P.bound_score[b] = bi == INT_MAX ? -INFINITY : bs;
        P.bound_item[b] = bi;
      }
    }
    if (l == bl) {
      ++p;
      hs = p < KM ? P.list_score[base + l * KM + p] : -INFINITY;
      hi = p < KM ? P.list_item[base + l * KM + p] : INT_MAX;
    }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// List depth: the shallower list when it needs no more passes than the deeper.
static int rec_km(int k) { return (k + 15) / 16 <= (k + 23) / 24 ? 16 : 24; }

struct RecLayout {
  size_t lscore, litem, bscore, bitem, total;
  long batch, splits;
  int km;
};

// `block_users`: users per workgroup of the scoring kernel.
static RecLayout rec_layout(long n_users, int n_items, int k, int cus, int block_users) {
  RecLayout L{};
  L.batch = n_users < FULL_BATCH ? n_users : FULL_BATCH;
  const size_t nb = (size_t)(L.batch > 0 ? L.batch : 1);   // (no users: a minimal layout)
  L.splits = full_splits((long)nb, n_items, cus, block_users);
  L.km = rec_km(k);
  const size_t n = nb * L.splits * 2 * L.km;
  Carver C;
  L.lscore = C.take_n<float>(n);
  L.litem = C.take_n<int>(n);
  L.bscore = C.take_n<float>(nb);
  L.bitem = C.take_n<int>(nb);
  L.total = C.used;
  return L;
}

template <int KM>
static int launch_rec_merge(const RecParams &P, long b0, int k, int pos0, int *topk,
                            float *topk_score, hipStream_t st) {
  const unsigned grid = (unsigned)((P.n_users + 3) / 4);
  const int n = k - pos0 < KM ? k - pos0 : KM;
  hipLaunchKernelGGL(recommend_merge_kernel<KM>, dim3(grid), dim3(256), 0, st, P, b0, k, pos0,
                     n, topk, topk_score);
  BBGR_LAUNCHED("recommend_merge_kernel");
  return BBGR_OK;
}

// The argument checks of bbgr_recommend and bbgr_recommend_bf16 (`Args`: either
// struct, the same field names). `ld_mult`: the row stride's multiple, 4 for
// fp32 tables and 8 for bf16 ones. BBGR_OK, or the refusal with its text set.
template <typename Args>
static int rec_check_args(const char *who, const Args *a, const size_t *workspace_bytes,
                          int ld_mult) {
  BBGR_REQUIRE_IN(who, a, "null args");
  BBGR_REQUIRE_IN(who, workspace_bytes, "null workspace_bytes");
  BBGR_REQUIRE_IN(who, a->n_users >= 0, "n_users < 0");
  BBGR_REQUIRE_IN(who, a->k >= 1 && a->k <= REC_MAX_K, "k not in [1, 128]");
  BBGR_REQUIRE_IN(who, a->n_items > 0, "n_items <= 0");
  BBGR_REQUIRE_IN(who, a->n_user_rows > 0, "n_user_rows <= 0");
  BBGR_REQUIRE_IN(who, (a->ex_indptr == nullptr) == (a->ex_indices == nullptr),
                  "ex_indptr and ex_indices must be given together");
  if (a->n_users > 0) {
    BBGR_REQUIRE_IN(who, a->users, "null users");
    BBGR_REQUIRE_IN(who, a->uf, "null uf");
    BBGR_REQUIRE_IN(who, a->itf, "null itf");
    BBGR_REQUIRE_IN(who, a->topk, "null topk");
  }
  BBGR_REQUIRE_IN(who, aligned16(a->uf) && a->lduf % ld_mult == 0,
                  ld_mult == 4 ? "uf must be 16-byte aligned, lduf % 4 == 0"
                               : "uf must be 16-byte aligned, lduf % 8 == 0");
  BBGR_REQUIRE_IN(who, aligned16(a->itf) && a->ldif % ld_mult == 0,
                  ld_mult == 4 ? "itf must be 16-byte aligned, ldif % 4 == 0"
                               : "itf must be 16-byte aligned, ldif % 8 == 0");
  const int d = a->d;
  if (d != 64 && d != 128 && d != 256) return unsupported_width(who, d, true);
  BBGR_REQUIRE_IN(who, a->n_users == 0 || (a->lduf >= d && a->ldif >= d), "lduf / ldif < d");
  return BBGR_OK;
}

// The body of both entry points after the checks: the size query, then per
// batch of users ceil(k / depth) scoring passes (`launch(P, depth, stream)`,
// the entry's own kernel), each followed by the merge.
template <typename Args, typename Launch>
static int rec_run(const char *who, const Args *a, void *workspace, size_t *workspace_bytes,
                   int block_users, bbgr_stream_t stream, Launch &&launch) {
  const RecLayout L = rec_layout(a->n_users, a->n_items, a->k, device_cus(), block_users);
  bool query;
  if (int rc = take_workspace(who, L.total, workspace, workspace_bytes, &query)) return rc;
  if (query) return BBGR_OK;
  hipStream_t st = as_stream(stream);
  for (long b0 = 0; b0 < a->n_users; b0 += L.batch) {
    RecParams P;
    P.n_users = a->n_users - b0 < L.batch ? a->n_users - b0 : L.batch;
    P.users = (const long *)a->users + b0;
    P.ex_indptr = a->ex_indptr;
    P.ex_indices = a->ex_indices;
    P.item_mask = a->item_mask;
    P.uf = a->uf;
    P.itf = a->itf;
    P.lduf = a->lduf;
    P.ldif = a->ldif;
    P.n_items = a->n_items;
    P.n_splits = (int)L.splits;
    const long per = (a->n_items + L.splits - 1) / L.splits;
    P.split_items = (int)((per + FULL_TILE - 1) / FULL_TILE * FULL_TILE);
    P.list_score = ws_at<float>(workspace, L.lscore);
    P.list_item = ws_at<int>(workspace, L.litem);
    P.bound_score = ws_at<float>(workspace, L.bscore);
    P.bound_item = ws_at<int>(workspace, L.bitem);
    for (int pos0 = 0; pos0 < a->k; pos0 += L.km) {
      P.cont = pos0 > 0;
      int rc = launch(P, L.km, st);
      if (rc) return rc;
      rc = L.km == 16 ? launch_rec_merge<16>(P, b0, a->k, pos0, a->topk, a->topk_score, st)
                      : launch_rec_merge<24>(P, b0, a->k, pos0, a->topk, a->topk_score, st);
      if (rc) return rc;
    }
  }
  return BBGR_OK;
}

}  // namespace bbgr
