// scan_words.h -- device code the item scans share (recommend.hip's fp32
// scan, twostage.hip's bf16 scan): the cut of a row's candidate buffer to its
// best k words.  A candidate is one 64-bit word, score_key(score) << 32 | ~id
// (recommend.hip).  Internal header.
#pragma once

#include "common.h"

namespace frecsys_hip {

// The `nn` (<= CAP) candidates of buffer g sorted (descending) by one wave in
// its LDS slice sb; the best min(nn, k) written back.  Returns that count;
// *kth = the k-th best word when nn >= k.
template <int CAP>
__device__ __forceinline__ int compact_row(unsigned long long* __restrict__ g,
                                           unsigned long long* sb, int nn, int k, int lane,
                                           unsigned long long* kth) {
  typedef unsigned long long u64;
  if (nn > CAP) nn = CAP;  // never: a row enters a tile with at most CAP - IT candidates
  int P = 64;
  while (P < nn) P <<= 1;
  for (int i = lane; i < P; i += 64) sb[i] = i < nn ? g[i] : 0ull;
  wave_lds_sync();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = lane; p < (P >> 1); p += 64) {
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i | stride;
        const bool up = (i & size) == 0;
        const u64 a = sb[i], b = sb[j];
        if (up ? a < b : a > b) {
          sb[i] = b;
          sb[j] = a;
        }
      }
      wave_lds_sync();
    }
  }
  const int keep = nn < k ? nn : k;
  for (int i = lane; i < keep; i += 64) g[i] = sb[i];
  if (nn >= k) *kth = sb[k - 1];
  wave_lds_sync();
  return keep;
}

}  // namespace frecsys_hip
