// What the two feature translation units share (features.hip,
// features_v2.hip): the row-length split, the rounded rating, the fixed-shape
// workgroup sum, an entropy term, and the host checks of the columns and of a
// row pass's workspace.
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

inline int feat_columns_ok(const char *fn, const bbgr_feat_columns *c) {
#define FEAT_REQ(cond, what)                          \
  do {                                                \
    if (!(cond)) {                                    \
      set_error("%s: %s", fn, what);                  \
      return BBGR_ERR_INVALID;                        \
    }                                                 \
  } while (0)
  FEAT_REQ(c, "null columns");
  FEAT_REQ(c->n >= 0 && c->n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  FEAT_REQ(c->n_users >= 0 && c->n_users < INT_MAX, "n_users out of range");
  FEAT_REQ(c->n_items >= 0, "n_items < 0");
  if (c->n == 0) return BBGR_OK;
  FEAT_REQ(c->n_users > 0 && c->n_items > 0, "records but no n_users / n_items");
  FEAT_REQ(c->user, "null user");
  FEAT_REQ(c->item, "null item");
  FEAT_REQ(c->rating, "null rating");
  FEAT_REQ(c->helpful_vote, "null helpful_vote");
  FEAT_REQ(c->verified, "null verified");
  FEAT_REQ(c->timestamp, "null timestamp");
  FEAT_REQ(c->n_tokens, "null n_tokens");
  FEAT_REQ(c->n_unique_tokens, "null n_unique_tokens");
#undef FEAT_REQ
  return BBGR_OK;
}

// Workspace of the two row passes: the long-row counter, then the list. A
// long row has more than FEAT_LONG_ROW records, so there are fewer than
// n / FEAT_LONG_ROW of them.
inline size_t feat_long_bytes(long n) {
  return align_up(256 + sizeof(int) * (size_t)(n / FEAT_LONG_ROW + 1));
}

inline int feat_workspace(const char *fn, size_t need, void *workspace, size_t *workspace_bytes,
                          bool *query) {
  *query = workspace == nullptr;
  if (!workspace) {
    *workspace_bytes = need;
    return BBGR_OK;
  }
  if (*workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", fn, *workspace_bytes, need);
    return BBGR_ERR_WORKSPACE;
  }
  return BBGR_OK;
}

}  // namespace bbgr
