// bbgr_text_gather: pack a list of variable-length records of a text of any
// size back to back (bbgr.text regroups the records by user with it, so that
// a chunk of bbgr_text_unique_pooled holds whole users).
//
// Three steps on the stream. text_gather_len_kernel, one lane per listed
// record: its clamped length (0 for an id outside [0, n)). hipcub's inclusive
// sum of the lengths behind out_offsets[0] = 0, and a copy of its last entry
// to total. text_gather_kernel, output-centric: the packed bytes are a flat
// array of 16-byte words and a wave owns GATHER_TILE = 1 KiB of it at a time,
// lane l word l. A wave takes a run of consecutive tiles. For the first it
// finds the record that holds the tile's first byte with a 64-ary search of
// out_offsets (every lane probes one entry, a ballot narrows the range 65
// times a step: 4 dependent loads for a million records where a binary search
// takes 20); from there on it walks: one coalesced load of the next 64 entries
// and a ballot give the last record of the tile and the first of the next. A
// lane finds its own record by a binary search inside that window (a review is
// a few hundred bytes: two or three entries) and assembles its word from one
// unaligned 16-byte load; where a record ends inside the word it moves on to
// the next record that has a byte, shifting each piece into place. So every
// store but the last partial word is a full aligned 16 bytes, and the work of
// a lane does not depend on how long the records are: a record of 1 MB is
// 65,536 words like any others.
//
// Reads stay inside data[first, last): a source position is checked against
// the range before its load, and the 16-byte load is taken only where all 16
// bytes lie below `last` (else the bytes are read one by one). Writes stay
// below min(total, capacity). Plain copies: two calls give the same bytes.
// bbgr_text_gather_fetch runs the same kernel with the other source fetch
// (the one or two aligned 16-byte words that hold the bytes, and a shift) for
// the measurement of DESIGN 4g (tools/text_bench.py --pooled --chunk-bytes).
#include "cub_temp.h"
#include "text.h"

namespace bbgr {

constexpr int GATHER_WAVES = 4;              // waves per workgroup of 256 threads
constexpr long GATHER_TILE = 1024;           // output bytes a wave writes per step: 16 a lane
constexpr long GATHER_TILES_PER_WAVE = 16;   // consecutive tiles per wave at a full capacity
constexpr long GATHER_MAX_BLOCKS = 32768;

typedef unsigned long long u64;
typedef unsigned __int128 u128;
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef u4v u4v_any __attribute__((aligned(1)));   // at any address: one unaligned 16-byte load

struct GatherParams {
  long n_list;
  const int *records;
  long n;
  const uint8_t *data;
  const long long *offsets;
  long first, last;
  long long *out_offsets;
  uint8_t *out_data;
  long capacity;
};

// The source bytes [beg, end) of listed record j: empty for an id outside
// [0, n) and for offsets that clamp to nothing; else inside [first, last).
__device__ __forceinline__ void gather_range(const GatherParams &P, long j, long &beg, long &end) {
  const long r = P.records[j];
  beg = end = 0;
  if (r < 0 || r >= P.n) return;
  text_range(P.offsets, r, P.first, P.last, beg, end);
  if (end < beg) end = beg;
}

__global__ __launch_bounds__(256) void text_gather_len_kernel(GatherParams P, long long *len) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.n_list) return;
  long beg, end;
  gather_range(P, j, beg, end);
  len[j] = end - beg;
}

// The largest j in [0, n_list) with off[j] <= target, for off[0] <= target <
// off[n_list]; called by the whole wave, the result is wave-uniform.
__device__ __forceinline__ long gather_find(const long long *off, long n_list, long target,
                                            int lane) {
  long lo = 0, hi = n_list;   // off[lo] <= target < off[hi]
  while (hi - lo > 1) {
    const long span = hi - lo;
    const long idx = lo + (long)(lane + 1) * span / 65;   // in [lo, hi), ascending over the lanes
    const int cnt = __popcll(__ballot((long)off[idx] <= target));   // a prefix of the lanes
    const long new_lo = cnt ? lo + (long)cnt * span / 65 : lo;
    hi = cnt < 64 ? lo + (long)(cnt + 1) * span / 65 : hi;
    lo = new_lo;
  }
  return lo;
}

// The same from a record `base` with off[base] <= target that lies close
// before the answer: 64 entries a step, one coalesced load.
__device__ __forceinline__ long gather_walk(const long long *off, long n_list, long base,
                                            long target, int lane) {
  for (;;) {
    const long idx = base + 1 + lane;
    const bool le = idx < n_list && (long)off[idx] <= target;   // off[n_list] > target
    const int cnt = __popcll(__ballot(le));
    base += cnt;
    if (cnt < 64) return base;
  }
}

__device__ __forceinline__ u128 gather_word(u4v v) {
  return (u128)((u64)v.x | (u64)v.y << 32) | (u128)((u64)v.z | (u64)v.w << 32) << 64;
}

// Up to 16 source bytes from position s as one little-endian 128-bit word.
// FETCH 0 (bbgr_text_gather): all 16 with one unaligned load where they lie
// below `last`. FETCH 1 (measured beside it): the one or two
// aligned 16-byte words that hold them and a byte shift, where both words lie
// inside data[first, last). Else the `want` bytes asked for, one by one.
// Nothing outside data[first, last) is read.
template <int FETCH>
__device__ __forceinline__ u128 gather_fetch(const GatherParams &P, long s, int want) {
  if (s < P.first || s >= P.last) return 0;
  if (FETCH == 0 && s + 16 <= P.last)
    return gather_word(*reinterpret_cast<const u4v_any *>(P.data + s));
  if (FETCH == 1) {
    const uint8_t *at = P.data + s;
    const int mis = (int)(reinterpret_cast<uintptr_t>(at) & 15u);
    const uint8_t *base = at - mis;
    if (base >= P.data + P.first && base + (mis ? 32 : 16) <= P.data + P.last) {
      const u128 lo = gather_word(*reinterpret_cast<const u4v *>(base));
      if (mis == 0) return lo;
      const u128 hi = gather_word(*reinterpret_cast<const u4v *>(base + 16));
      return lo >> (8 * mis) | hi << (8 * (16 - mis));
    }
  }
  const long have = P.last - s;
  const int cnt = want < have ? want : (int)have;
  u128 w = 0;
  for (int k = cnt - 1; k >= 0; --k) w = w << 8 | (u128)P.data[s + k];   // the last byte first
  return w;
}

// The first `take` (1 .. 16) bytes of w, moved up by `at` (0 .. 15) bytes.
__device__ __forceinline__ u128 gather_place(u128 w, int take, int at) {
  if (take < 16) w &= ((u128)1 << (8 * take)) - 1;
  return w << (8 * at);
}

template <int FETCH>
__global__ __launch_bounds__(64 * GATHER_WAVES) void text_gather_kernel(GatherParams P) {
  const int lane = threadIdx.x & 63;
  const long wave =   // wave-uniform, and known to be
      __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6)));
  const long n_waves = (long)gridDim.x * GATHER_WAVES;
  const long long *off = P.out_offsets;
  const long total = (long)off[P.n_list];
  const long lim = total < P.capacity ? total : P.capacity;   // no byte at or behind it is written
  if (lim <= 0) return;
  const long n_tiles = (lim + GATHER_TILE - 1) / GATHER_TILE;
  const long per = (n_tiles + n_waves - 1) / n_waves;
  long tile = wave * per;
  const long tile_end = tile + per < n_tiles ? tile + per : n_tiles;
  if (tile >= tile_end) return;
  long j_lo = gather_find(off, P.n_list, tile * GATHER_TILE, lane);
  for (; tile < tile_end; ++tile) {
    const long t0 = tile * GATHER_TILE;
    const long t1 = t0 + GATHER_TILE < lim ? t0 + GATHER_TILE : lim;
    const long j_hi = gather_walk(off, P.n_list, j_lo, t1 - 1, lane);
    const long p = t0 + 16 * lane;   // this lane's word
    if (p < t1) {
      long a = j_lo, b = j_hi;   // the record that holds byte p: the last with off[j] <= p
      while (a < b) {
        const long mid = (a + b + 1) >> 1;
        if ((long)off[mid] <= p) a = mid;
        else b = mid - 1;
      }
      long j = a;
      const int need = t1 - p < 16 ? (int)(t1 - p) : 16;
      u128 w = 0;
      int filled = 0;
      for (;;) {
        const long rec_beg = (long)off[j], rec_end = (long)off[j + 1];
        const long pos = p + filled;
        const long left = rec_end - pos;
        const int take = left < need - filled ? (int)left : need - filled;
        if (take <= 0) break;   // never, with offsets this call has scanned itself
        long s_beg, s_end;
        gather_range(P, j, s_beg, s_end);
        w |= gather_place(gather_fetch<FETCH>(P, s_beg + (pos - rec_beg), take), take, filled);
        filled += take;
        if (filled >= need) break;
        // the next record that has a byte: there is one, pos + take < lim <= off[n_list]
        if (++j >= P.n_list) break;
        while (j + 1 < P.n_list && off[j + 1] == off[j]) ++j;
      }
      if (need == 16) {
        u4v v;
        v.x = (unsigned)w;
        v.y = (unsigned)(w >> 32);
        v.z = (unsigned)(w >> 64);
        v.w = (unsigned)(w >> 96);
        *reinterpret_cast<u4v *>(P.out_data + p) = v;
      } else {
        for (int k = 0; k < need; ++k) {   // the last partial word of the output
          P.out_data[p + k] = (uint8_t)w;
          w >>= 8;
        }
      }
    }
    if (tile + 1 < tile_end) j_lo = gather_walk(off, P.n_list, j_hi, t1, lane);
  }
}

}  // namespace bbgr

using namespace bbgr;

// bbgr_text_gather, or (tools/text_bench.py) the same with the other source fetch.
static int text_gather(const char *fn, const bbgr_text_gather_args *a, int fetch, void *workspace,
                       size_t *workspace_bytes, bbgr_stream_t stream) {
  BBGR_REQUIRE_IN(fn, a, "null args");
  BBGR_REQUIRE_IN(fn, a->n_list >= 0 && a->n_list < 2147483647LL,
                  "n_list out of range (n_list must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, a->n >= 0, "n < 0");
  BBGR_REQUIRE_IN(fn, a->first >= 0, "first < 0");
  BBGR_REQUIRE_IN(fn, a->last >= a->first, "last < first");
  BBGR_REQUIRE_IN(fn, a->capacity >= 0, "capacity < 0");
  BBGR_REQUIRE_IN(fn, aligned16(a->out_data), "out_data must be 16-byte aligned");
  if (a->n_list > 0) {
    BBGR_REQUIRE_IN(fn, a->records, "null records");
    BBGR_REQUIRE_IN(fn, a->out_offsets, "null out_offsets");
    BBGR_REQUIRE_IN(fn, a->total, "null total");
    if (a->n > 0) {
      BBGR_REQUIRE_IN(fn, a->data, "null data");
      BBGR_REQUIRE_IN(fn, a->offsets, "null offsets");
    }
  }
  const long n_list = (long)a->n_list;
  Carver C;
  const size_t off_len = C.take_n<long long>((size_t)n_list);
  const size_t temp =
      n_list > 0 ? hcub::inclusive_sum_temp<const long long *, long long *>((int)n_list) : 0;
  const size_t off_tmp = C.take(temp);
  bool query;
  int rc = take_workspace(fn, C.used, workspace, workspace_bytes, &query);
  if (rc || query || n_list == 0) return rc;
  hipStream_t st = as_stream(stream);
  GatherParams P;
  P.n_list = n_list;
  P.records = a->records;
  P.n = (long)a->n;
  P.data = a->data;
  P.offsets = reinterpret_cast<const long long *>(a->offsets);
  P.first = (long)a->first;
  P.last = (long)a->last;
  P.out_offsets = reinterpret_cast<long long *>(a->out_offsets);
  P.out_data = a->out_data;
  P.capacity = (long)a->capacity;
  long long *len = ws_at<long long>(workspace, off_len);
  hipLaunchKernelGGL(text_gather_len_kernel, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0,
                     st, P, len);
  BBGR_LAUNCHED("text_gather_len_kernel");
  BBGR_HIP(hipMemsetAsync(P.out_offsets, 0, sizeof(long long), st));
  BBGR_HIP(hcub::inclusive_sum(ws_at<char>(workspace, off_tmp), temp, (const long long *)len,
                               P.out_offsets + 1, (int)n_list, st));
  BBGR_HIP(hipMemcpyAsync(a->total, P.out_offsets + n_list, sizeof(long long),
                          hipMemcpyDeviceToDevice, st));
  if (!a->out_data || a->capacity == 0) return BBGR_OK;
  const long cap_tiles = (P.capacity + GATHER_TILE - 1) / GATHER_TILE;
  const long per_block = GATHER_WAVES * GATHER_TILES_PER_WAVE;
  long blocks = (cap_tiles + per_block - 1) / per_block;
  blocks = blocks < GATHER_MAX_BLOCKS ? blocks : GATHER_MAX_BLOCKS;
  if (fetch == BBGR_TEXT_FETCH_UNALIGNED)
    hipLaunchKernelGGL(text_gather_kernel<0>, dim3((unsigned)blocks), dim3(64 * GATHER_WAVES), 0,
                       st, P);
  else
    hipLaunchKernelGGL(text_gather_kernel<1>, dim3((unsigned)blocks), dim3(64 * GATHER_WAVES), 0,
                       st, P);
  BBGR_LAUNCHED("text_gather_kernel");
  return BBGR_OK;
}

extern "C" int bbgr_text_gather(const bbgr_text_gather_args *a, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  return text_gather("bbgr_text_gather", a, BBGR_TEXT_FETCH_UNALIGNED, workspace, workspace_bytes,
                     stream);
}

extern "C" int bbgr_text_gather_fetch(const bbgr_text_gather_args *a, int32_t fetch,
                                      void *workspace, size_t *workspace_bytes,
                                      bbgr_stream_t stream) {
  static const char *fn = "bbgr_text_gather_fetch";
  BBGR_REQUIRE_IN(fn, fetch == BBGR_TEXT_FETCH_UNALIGNED || fetch == BBGR_TEXT_FETCH_ALIGNED_PAIR,
                  "fetch out of range (0 .. 1)");
  return text_gather(fn, a, fetch, workspace, workspace_bytes, stream);
}
