// sba_ext.hpp — what the points + extrinsics SBA (sba_ext.hip) and its covariance
// (sba_ext_cov.hip) share.
#pragma once

#include <algorithm>

#include "common.hpp"

#define EXT_MAXC 16
#define EXT_CHUNK 64

__device__ __forceinline__ int upk(int i, int j) {  // packed upper-triangular index, 6x6
  if (i > j) {
    const int t = i;
    i = j;
    j = t;
  }
  return i * 6 - i * (i - 1) / 2 + (j - i);
}

// points per Schur block: the W M tiles of a chunk (18 doubles and a camera id per slot, 3
// doubles per point) must fit ~96 KB of LDS
static inline int ext_chunk_points(int K) { return std::max(1, std::min(EXT_CHUNK, (int)(96 * 1024 / (148 * K + 24)))); }
