// The hipcub primitives the entry points use, each as a pair: NAME_temp(...)
// returns the temporary storage the primitive needs (what hipcub answers to a
// null temp pointer: no launch, a null stream), NAME(temp, bytes, ...) runs it
// on the caller's stream with the size passed by value. The _temp forms take
// the pointer / iterator types of the run as template arguments (null
// pointers, value-initialised), so sizing and run instantiate one hipcub
// template.
//
// hipcub asks the runtime for a device while it sizes some primitives (every
// scan, DeviceSelect::If, the larger radix sorts): without one the size comes
// back 0 and `*err` (optional) holds the runtime's error. Entry points whose
// size query reports that error pass `err`; the others size on any host.
#pragma once

#include <hipcub/hipcub.hpp>

#include "common.h"

namespace bbgr {
namespace hcub {

constexpr hipStream_t NO_STREAM = nullptr;

// The bytes a sizing call left in `b`, its status into *err (optional).
struct Sizing {
  hipError_t *err;
  size_t b = 0;
  size_t done(hipError_t e) {
    if (err) *err = e;
    return b;
  }
};

template <class In, class Out>
size_t exclusive_sum_temp(int n, hipError_t *err = nullptr, In in = In{}) {
  Sizing s{err};
  return s.done(hipcub::DeviceScan::ExclusiveSum(nullptr, s.b, in, Out{}, n, NO_STREAM));
}
template <class In, class Out>
hipError_t exclusive_sum(void *temp, size_t bytes, In in, Out out, int n, hipStream_t st) {
  return hipcub::DeviceScan::ExclusiveSum(temp, bytes, in, out, n, st);
}

template <class In, class Out>
size_t inclusive_sum_temp(int n, hipError_t *err = nullptr, In in = In{}) {
  Sizing s{err};
  return s.done(hipcub::DeviceScan::InclusiveSum(nullptr, s.b, in, Out{}, n, NO_STREAM));
}
template <class In, class Out>
hipError_t inclusive_sum(void *temp, size_t bytes, In in, Out out, int n, hipStream_t st) {
  return hipcub::DeviceScan::InclusiveSum(temp, bytes, in, out, n, st);
}

template <class K, class V>
size_t sort_pairs_temp(int n, int begin_bit, int end_bit, hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceRadixSort::SortPairs(nullptr, s.b, (const K *)nullptr, (K *)nullptr,
      (const V *)nullptr, (V *)nullptr, n, begin_bit, end_bit, NO_STREAM));
}
template <class K, class V>
hipError_t sort_pairs(void *temp, size_t bytes, const K *k_in, K *k_out, const V *v_in, V *v_out,
                      int n, int begin_bit, int end_bit, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairs(temp, bytes, k_in, k_out, v_in, v_out, n, begin_bit,
                                            end_bit, st);
}

template <class K, class V>
size_t sort_pairs_descending_temp(int n, int begin_bit, int end_bit, hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, s.b, (const K *)nullptr,
      (K *)nullptr, (const V *)nullptr, (V *)nullptr, n, begin_bit, end_bit, NO_STREAM));
}
template <class K, class V>
hipError_t sort_pairs_descending(void *temp, size_t bytes, const K *k_in, K *k_out, const V *v_in,
                                 V *v_out, int n, int begin_bit, int end_bit, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairsDescending(temp, bytes, k_in, k_out, v_in, v_out, n,
                                                      begin_bit, end_bit, st);
}

template <class K>
size_t sort_keys_temp(int n, int begin_bit, int end_bit, hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceRadixSort::SortKeys(nullptr, s.b, (const K *)nullptr, (K *)nullptr,
      n, begin_bit, end_bit, NO_STREAM));
}
template <class K>
hipError_t sort_keys(void *temp, size_t bytes, const K *k_in, K *k_out, int n, int begin_bit,
                     int end_bit, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortKeys(temp, bytes, k_in, k_out, n, begin_bit, end_bit, st);
}

// Segmented radix sorts: `n` items in `segments` segments [seg_b[s], seg_e[s]).
template <class K, class V, class Seg>
size_t seg_sort_pairs_temp(int n, int segments, Seg seg_b, Seg seg_e, int begin_bit, int end_bit,
                           hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, s.b, (const K *)nullptr,
      (K *)nullptr, (const V *)nullptr, (V *)nullptr, n, segments, seg_b, seg_e, begin_bit,
      end_bit, NO_STREAM));
}
template <class K, class V, class Seg>
hipError_t seg_sort_pairs(void *temp, size_t bytes, const K *k_in, K *k_out, const V *v_in,
                          V *v_out, int n, int segments, Seg seg_b, Seg seg_e, int begin_bit,
                          int end_bit, hipStream_t st) {
  return hipcub::DeviceSegmentedRadixSort::SortPairs(temp, bytes, k_in, k_out, v_in, v_out, n,
                                                     segments, seg_b, seg_e, begin_bit, end_bit, st);
}

template <class K, class Seg>
size_t seg_sort_keys_temp(int n, int segments, Seg seg_b, Seg seg_e, int begin_bit, int end_bit,
                          hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, s.b, (const K *)nullptr,
      (K *)nullptr, n, segments, seg_b, seg_e, begin_bit, end_bit, NO_STREAM));
}
template <class K, class Seg>
hipError_t seg_sort_keys(void *temp, size_t bytes, const K *k_in, K *k_out, int n, int segments,
                         Seg seg_b, Seg seg_e, int begin_bit, int end_bit, hipStream_t st) {
  return hipcub::DeviceSegmentedRadixSort::SortKeys(temp, bytes, k_in, k_out, n, segments, seg_b,
                                                    seg_e, begin_bit, end_bit, st);
}

template <class Out, class Count, class In, class Op>
size_t select_if_temp(In in, int n, Op op, hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceSelect::If(nullptr, s.b, in, Out{}, Count{}, n, op, NO_STREAM));
}
template <class In, class Out, class Count, class Op>
hipError_t select_if(void *temp, size_t bytes, In in, Out out, Count count, int n, Op op,
                     hipStream_t st) {
  return hipcub::DeviceSelect::If(temp, bytes, in, out, count, n, op, st);
}

template <class In, class Uniq, class Len, class Runs>
size_t run_length_encode_temp(int n, hipError_t *err = nullptr) {
  Sizing s{err};
  return s.done(hipcub::DeviceRunLengthEncode::Encode(nullptr, s.b, In{}, Uniq{}, Len{}, Runs{}, n,
      NO_STREAM));
}
template <class In, class Uniq, class Len, class Runs>
hipError_t run_length_encode(void *temp, size_t bytes, In in, Uniq uniq, Len len, Runs runs, int n,
                             hipStream_t st) {
  return hipcub::DeviceRunLengthEncode::Encode(temp, bytes, in, uniq, len, runs, n, st);
}

}  // namespace hcub
}  // namespace bbgr
