// Device helpers shared by the full-ranking scorers (eval.hip's
// eval_full_kernel, recommend.hip's recommend_kernel): the binary search of a
// sorted CSR row, the sorted register list, the MFMA accumulator type and the
// item-split rule of a small user batch.
#pragma once

#include "common.h"

namespace bbgr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FULL_TILE = 128;         // items per full-ranking LDS tile (d = 64)
constexpr long FULL_BATCH = 1l << 18;  // users per full-ranking launch

__device__ __forceinline__ int lower_bound_i32(const int *a, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One (score, item) into a sorted register list (score desc, item asc).
template <int KM>
__device__ __forceinline__ void topk_insert(float (&tv)[KM], int (&ti)[KM], float s, int it) {
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    const bool sw = s > tv[j] || (s == tv[j] && it < ti[j]);
    const float t = tv[j];
    const int q = ti[j];
    tv[j] = sw ? s : t;
    ti[j] = sw ? it : q;
    s = sw ? t : s;
    it = sw ? q : it;
  }
}

// Item splits so that small user counts still fill the chip (>= 4 workgroups
// per CU at `block_users` users per workgroup), each split at least 4 tiles,
// at most 32 (merge: 2 lists per split on one wave).
inline long full_splits(long n_users, int n_items, int cus, int block_users) {
  const long blocks = (n_users + block_users - 1) / block_users;
  const long want = 4l * cus;
  long s = blocks >= want ? 1 : (want + blocks - 1) / blocks;
  const long max_s = (n_items + FULL_TILE * 4 - 1) / (FULL_TILE * 4);
  s = s > max_s ? max_s : s;
  s = s > 32 ? 32 : s;
  return s < 1 ? 1 : s;
}

inline int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
      cus = p.multiProcessorCount;
  }
  return cus;
}

}  // namespace bbgr
