// Token and distinct-token counts of review text
// (main.py tokenize(): re.findall(r"[a-z]+(?:'[a-z]+)?", s.lower())), over
// the UTF-8 bytes of the records.
//
// The rule over bytes. A letter is an ASCII A-Za-z, or the byte C4 when B0
// follows it inside the record (U+0130, whose lower() is "i" + U+0307: C4 is
// the letter i, B0 a separator). 0x27 is the apostrophe. Every other byte is
// a separator, and so is a record's edge. A maximal run of letters is attached
// when the byte before it is an apostrophe and the byte before that a letter.
// A run begins a token unless it is attached and the run before it began one;
// then it is that token's apostrophe part. U+212A (E2 84 AA, whose lower() is
// "k") is the one letter that is not one byte: the kernels read its bytes as
// separators and bbgr_text_count flags every record that holds it (recheck),
// for the caller to count on the host.
//
// text_walk_kernel: one wave per record, TEXT_STEP = 64 bytes a step, lane l
// byte l of the step: one coalesced 64-byte read. Ballots of the two classes
// give a letter mask L and an apostrophe mask A; shifted by one and two, with
// the last two bytes of the step before carried in three bits, they give the
// run starts S = L & ~L1 and the attached starts S & A1 & L2. The chain
// "attached and the run before began a token" is resolved on the masks in a
// wave-uniform loop over the attached starts alone (none in most steps); the
// fourth carried bit says whether the last run start began a token. The same
// kernel, EMIT, writes every token's start and record at its slot
// tok_off[record] + rank.
//
// bbgr_text_unique: given a token's start its extent follows forward (its run,
// then "'" + the next run if one is attached), so the per-token kernels walk
// from the start: text_hash_kernel one lane per token (FNV-1a over the
// normalised bytes, then a finaliser, masked), hipcub's segmented radix sort
// by hash inside each record (stable: equal hashes stay in text order), and
// text_verify_kernel one lane per sorted slot: a slot opens a new distinct
// token when its hash differs from its left neighbour's; with equal hashes
// the two tokens' normalised bytes are compared to their ends, and any
// difference flags the record. In an unflagged record every run of equal
// hashes is therefore one string and the count is exact.
//
// Integer work only; the integer atomics add order-free sums: two calls give
// the same bits. Measured in DESIGN 4f (tools/text_bench.py).
#include "cub_temp.h"
#include "text.h"

#include <limits.h>

namespace bbgr {

constexpr int TEXT_STEP = 64;          // bytes of a record one wave reads per step: a byte a lane
constexpr int TEXT_WAVES = 4;          // records in flight per workgroup of 256 threads
constexpr long TEXT_MAX_BLOCKS = 16384;

struct TextParams {
  long n;
  const uint8_t *data;
  const long long *offsets;
  long first, last;
  int *n_tokens;
  uint8_t *recheck;
  long long *totals;
  // EMIT
  const int *tok_off;   // [n + 1]
  uint32_t *tok_pos;    // [total]: the token's first byte, relative to `first`
  int *tok_rec;         // [total]
  long total;
};

template <bool EMIT>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_walk_kernel(TextParams P) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6);
  const long n_waves = (long)gridDim.x * TEXT_WAVES;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long wave_tokens = 0;
  for (long r = wave; r < P.n; r += n_waves) {
    long beg, end;
    text_range(P.offsets, r, P.first, P.last, beg, end);
    // carried over a step edge (wave-uniform): the classes of the last two
    // bytes, whether the last run start began a token, the last two bytes
    unsigned long long pL1 = 0, pA1 = 0, pL2 = 0;
    bool last_began = false;
    unsigned t1 = 0, t2 = 0;   // bytes at -1 and -2 of this step
    bool kelvin = false;
    int count = 0;
    const int slot0 = EMIT ? P.tok_off[r] : 0;
    for (long base = beg; base < end; base += TEXT_STEP) {
      const long p = base + lane;
      const unsigned b = p < end ? P.data[p] : 0u;
      unsigned nb = __shfl_down(b, 1);
      if (lane == 63) nb = p + 1 < end ? P.data[p + 1] : 0u;
      const bool is_l = text_ascii_letter(b) || (b == 0xC4u && nb == 0xB0u);
      const unsigned long long L = __ballot(is_l), A = __ballot(b == 0x27u);
      // U+212A: AA after 84 after E2, over step edges by the carried bytes
      unsigned b1 = __shfl_up(b, 1), b2 = __shfl_up(b, 2);
      if (lane == 0) b1 = t1;
      if (lane == 0) b2 = t2;
      if (lane == 1) b2 = t1;
      kelvin |= __ballot(b == 0xAAu && b1 == 0x84u && b2 == 0xE2u) != 0ull;
      const unsigned long long L1 = L << 1 | pL1, A1 = A << 1 | pA1,
                               L2 = L << 2 | pL1 << 1 | pL2;
      const unsigned long long S = L & ~L1;
      unsigned long long att = S & A1 & L2, B = S;
      while (att) {   // wave-uniform, in text order
        const int i = __ffsll((long long)att) - 1;
        att &= att - 1;
        const unsigned long long before = S & ((1ull << i) - 1ull);
        const bool prev_began = before ? (B >> (63 - __clzll((long long)before)) & 1ull) != 0ull
                                       : last_began;
        if (prev_began) B &= ~(1ull << i);
      }
      if (S) last_began = (B >> (63 - __clzll((long long)S)) & 1ull) != 0ull;
      if (EMIT && (B >> lane & 1ull)) {
        const long slot = (long)slot0 + count + __popcll(B & below);
        if (slot >= 0 && slot < P.total) {   // always, when total is the count pass's own sum
          P.tok_pos[slot] = (uint32_t)(p - P.first);
          P.tok_rec[slot] = (int)r;
        }
      }
      count += __popcll(B);
      pL1 = L >> 63;
      pA1 = A >> 63;
      pL2 = L >> 62 & 1ull;
      t1 = __shfl(b, 63);
      t2 = __shfl(b, 62);
    }
    if (!EMIT && lane == 0) {
      P.n_tokens[r] = count;
      P.recheck[r] = kelvin ? 1 : 0;
    }
    wave_tokens += count;
  }
  if (!EMIT && lane == 0 && wave_tokens)
    atomicAdd(reinterpret_cast<unsigned long long *>(P.totals), (unsigned long long)wave_tokens);
}

__global__ __launch_bounds__(256) void text_hash_kernel(TextTokens T, unsigned long long *keys,
                                                        uint32_t *vals) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= text_live_tokens(T)) return;
  TokenCursor c = text_cursor(T, t);
  unsigned long long h = 0xcbf29ce484222325ull;   // FNV-1a, 64 bits
  for (int ch = c.next(); ch >= 0; ch = c.next()) h = (h ^ (unsigned long long)ch) * 0x100000001b3ull;
  h ^= h >> 29;   // finaliser: the high bits reach the low ones a narrow mask keeps
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  keys[t] = h & T.hash_mask;
  vals[t] = (uint32_t)t;
}

// One lane per sorted slot. n_unique_tokens was zeroed; the lanes of a wave
// that share a record add their count with one integer atomic.
__global__ __launch_bounds__(256) void text_verify_kernel(TextTokens T,
                                                          const unsigned long long *keys,
                                                          const uint32_t *vals, int *n_unique,
                                                          uint8_t *recheck) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  int rec = j < text_live_tokens(T) ? T.tok_rec[j] : -1;   // the same before and after the sort
  if (rec >= T.n) rec = -1;
  const bool live = rec >= 0;
  bool opens = false;
  if (live) {
    opens = j == 0 || j == (long)T.tok_off[rec] || keys[j] != keys[j - 1];
    // every writer stores the same value
    if (!opens && text_tokens_differ(T, vals[j], vals[j - 1])) recheck[rec] = 1;
  }
  text_count_opens(rec, live, opens, n_unique);
}

__global__ __launch_bounds__(256) void text_recheck_total_kernel(long n, const uint8_t *recheck,
                                                                long long *totals) {
  long cnt = 0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long)gridDim.x * 256)
    cnt += recheck[r] != 0;
#pragma unroll
  for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt)
    atomicAdd(reinterpret_cast<unsigned long long *>(totals) + 1, (unsigned long long)cnt);
}

// Segment bounds of the sort: record r's tokens, by the token offsets.
typedef hipcub::TransformInputIterator<int, RowBound, hipcub::CountingInputIterator<int>> SegIter;

static unsigned text_walk_blocks(long n) {
  const long b = (n + TEXT_WAVES - 1) / TEXT_WAVES;
  return (unsigned)(b < TEXT_MAX_BLOCKS ? b : TEXT_MAX_BLOCKS);
}

static TextParams text_params(const bbgr_text_args *a) {
  TextParams P;
  P.n = (long)a->n;
  P.data = a->data;
  P.offsets = reinterpret_cast<const long long *>(a->offsets);
  P.first = (long)a->first;
  P.last = (long)a->last;
  P.n_tokens = a->n_tokens;
  P.recheck = a->recheck;
  P.totals = reinterpret_cast<long long *>(a->totals);
  P.tok_off = nullptr;
  P.tok_pos = nullptr;
  P.tok_rec = nullptr;
  P.total = 0;
  return P;
}

int text_check(const char *fn, const bbgr_text_args *a) {
  BBGR_REQUIRE_IN(fn, a, "null args");
  BBGR_REQUIRE_IN(fn, a->n >= 0 && a->n < 2147483647LL, "n out of range (n must be < 2^31 - 1)");
  BBGR_REQUIRE_IN(fn, a->first >= 0, "first < 0");
  BBGR_REQUIRE_IN(fn, a->last >= a->first, "last < first");
  BBGR_REQUIRE_IN(fn, a->last - a->first < 2147483647LL,
                  "last - first out of range (must be < 2^31 - 1 bytes)");
  if (a->n > 0) {
    BBGR_REQUIRE_IN(fn, a->data, "null data");
    BBGR_REQUIRE_IN(fn, a->offsets, "null offsets");
    BBGR_REQUIRE_IN(fn, a->n_tokens, "null n_tokens");
    BBGR_REQUIRE_IN(fn, a->n_unique_tokens, "null n_unique_tokens");
    BBGR_REQUIRE_IN(fn, a->recheck, "null recheck");
    BBGR_REQUIRE_IN(fn, a->totals, "null totals");
  }
  return BBGR_OK;
}

int text_flag_total(long n, const uint8_t *flag, int64_t *totals, hipStream_t st) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(text_recheck_total_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)),
                     dim3(256), 0, st, n, flag, reinterpret_cast<long long *>(totals));
  BBGR_LAUNCHED("text_recheck_total_kernel");
  return BBGR_OK;
}

}  // namespace bbgr

using namespace bbgr;

extern "C" int bbgr_text_count(const bbgr_text_args *a, bbgr_stream_t stream) {
  static const char *fn = "bbgr_text_count";
  if (int rc = text_check(fn, a)) return rc;
  if (a->n == 0) return BBGR_OK;
  hipStream_t st = as_stream(stream);
  BBGR_HIP(hipMemsetAsync(a->totals, 0, 2 * sizeof(int64_t), st));
  hipLaunchKernelGGL(text_walk_kernel<false>, dim3(text_walk_blocks((long)a->n)),
                     dim3(64 * TEXT_WAVES), 0, st, text_params(a));
  BBGR_LAUNCHED("text_walk_kernel<count>");
  return BBGR_OK;
}

// bbgr_text_unique, or (tools/text_bench.py) some of its launch groups on a
// workspace the groups before them have filled.
static int text_unique(const char *fn, const bbgr_text_args *a, int64_t total_tokens, int stages,
                       void *workspace, size_t *workspace_bytes, bbgr_stream_t stream) {
  if (int rc = text_check(fn, a)) return rc;
  // inside a record two tokens have a byte between them: a record of len bytes
  // holds at most (len + 1) / 2 tokens; a record's edge separates for free
  BBGR_REQUIRE_IN(fn, total_tokens >= 0 && total_tokens <= (a->last - a->first + a->n) / 2,
                  "total_tokens out of range (at most (last - first + n) / 2)");
  const long n = (long)a->n;
  const int T = (int)total_tokens;
  const size_t nt = (size_t)T;
  size_t t_scan = 0, t_sort = 0;
  if (n > 0) {
    t_scan = hcub::inclusive_sum_temp<const int *, int *>((int)n);
    const hipcub::CountingInputIterator<int> rec(0);
    const SegIter seg_b(rec, RowBound{nullptr, T, false}), seg_e(rec, RowBound{nullptr, T, true});
    t_sort = hcub::seg_sort_pairs_temp<unsigned long long, uint32_t>(T, (int)n, seg_b, seg_e, 0, 64);
  }
  const TextWorkspace W = text_workspace(n, nt);
  const size_t temp = t_scan > t_sort ? t_scan : t_sort;
  bool query;
  int rc = take_workspace(fn, W.off_tmp + align_up(temp), workspace, workspace_bytes, &query);
  if (rc || query || n == 0) return rc;
  hipStream_t st = as_stream(stream);
  int *tok_off = ws_at<int>(workspace, W.off_tok);
  int *tok_rec = ws_at<int>(workspace, W.off_rec);
  uint32_t *tok_pos = ws_at<uint32_t>(workspace, W.off_pos);
  unsigned long long *k1 = ws_at<unsigned long long>(workspace, W.off_k1);
  unsigned long long *k2 = ws_at<unsigned long long>(workspace, W.off_k2);
  uint32_t *v1 = ws_at<uint32_t>(workspace, W.off_v1), *v2 = ws_at<uint32_t>(workspace, W.off_v2);
  void *tmp = ws_at<char>(workspace, W.off_tmp);
  const TextTokens K = text_tokens(a, workspace, W, T);
  const unsigned tok_blocks = (unsigned)(((long)T + 255) / 256);
  if (T > 0 && (stages & BBGR_TEXT_STAGE_EMIT)) {
    // token offsets: tok_off[0] = 0, tok_off[r + 1] = n_tokens[0] + .. + n_tokens[r]
    BBGR_HIP(hipMemsetAsync(tok_off, 0, sizeof(int), st));
    BBGR_HIP(hcub::inclusive_sum(tmp, temp, (const int *)a->n_tokens, tok_off + 1, (int)n, st));
    TextParams P = text_params(a);
    P.tok_off = tok_off;
    P.tok_pos = tok_pos;
    P.tok_rec = tok_rec;
    P.total = T;
    hipLaunchKernelGGL(text_walk_kernel<true>, dim3(text_walk_blocks(n)), dim3(64 * TEXT_WAVES), 0,
                       st, P);
    BBGR_LAUNCHED("text_walk_kernel<emit>");
    hipLaunchKernelGGL(text_hash_kernel, dim3(tok_blocks), dim3(256), 0, st, K, k1, v1);
    BBGR_LAUNCHED("text_hash_kernel");
  }
  if (T > 0 && (stages & BBGR_TEXT_STAGE_SORT)) {
    const hipcub::CountingInputIterator<int> rec(0);
    const SegIter seg_b(rec, RowBound{tok_off, T, false}), seg_e(rec, RowBound{tok_off, T, true});
    BBGR_HIP(hcub::seg_sort_pairs(tmp, temp, (const unsigned long long *)k1, k2,
                                  (const uint32_t *)v1, v2, T, (int)n, seg_b, seg_e, 0, 64, st));
  }
  if (!(stages & BBGR_TEXT_STAGE_VERIFY)) return BBGR_OK;
  BBGR_HIP(hipMemsetAsync(a->n_unique_tokens, 0, sizeof(int) * (size_t)n, st));
  BBGR_HIP(hipMemsetAsync(a->totals + 1, 0, sizeof(int64_t), st));
  if (T > 0) {
    hipLaunchKernelGGL(text_verify_kernel, dim3(tok_blocks), dim3(256), 0, st, K,
                       (const unsigned long long *)k2, (const uint32_t *)v2, a->n_unique_tokens,
                       a->recheck);
    BBGR_LAUNCHED("text_verify_kernel");
  }
  return text_flag_total(n, a->recheck, a->totals, st);
}

extern "C" int bbgr_text_unique(const bbgr_text_args *a, int64_t total_tokens, void *workspace,
                                size_t *workspace_bytes, bbgr_stream_t stream) {
  return text_unique("bbgr_text_unique", a, total_tokens, BBGR_TEXT_STAGE_ALL, workspace,
                     workspace_bytes, stream);
}

extern "C" int bbgr_text_unique_stages(const bbgr_text_args *a, int64_t total_tokens,
                                       int32_t stages, void *workspace, size_t *workspace_bytes,
                                       bbgr_stream_t stream) {
  static const char *fn = "bbgr_text_unique_stages";
  BBGR_REQUIRE_IN(fn, stages > 0 && stages <= BBGR_TEXT_STAGE_ALL, "stages out of range (1 .. 7)");
  return text_unique(fn, a, total_tokens, stages, workspace, workspace_bytes, stream);
}
