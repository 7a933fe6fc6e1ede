// The keyframe database's place-recognition query (KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates,
// KeyFrameDatabase.cc:806-1089): for every keyframe of the database, against one query BowVector, the number of shared words, the
// first shared word and DBoW2's L1 score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) with the reference's own bits.
#include "kernels.hpp"
#include "device_prims.hpp"

namespace pli {

// One wave per slot, the slots strided over the waves of the grid.  The block stages the query's word ids in LDS (nq * 4 bytes,
// at most 32 KiB: PLI_BOW_MAX_FEATURES words); the query's values are read through L2 at the hits only.
//
// A wave walks its keyframe's words in chunks of 64, one word per lane (consecutive words and values: the loads coalesce), and
// every lane looks its word up in the staged query by bisection.  Both vectors ascend strictly, so the hits of a wave, taken chunk
// after chunk and lane after lane, are the shared words in ascending order — the order in which L1Scoring::score adds its terms.
// Each hit lane computes its own term fabs(vi - wi) - fabs(vi) - fabs(wi) (vi the query's value, wi the keyframe's: the operands
// do not commute in the last bit); only the additions are serial: the ballot of the hits is walked from its lowest bit, each term
// is brought to all lanes and added to an accumulator that every lane keeps.  No tree, no atomics, no reordering; the term holds
// no product, so nothing could contract either (-ffp-contract=off is set for the whole library).
__global__ __launch_bounds__(KFDB_QUERY_BLOCK) void k_kfdb_query(const uint32_t* __restrict__ qWord, const double* __restrict__ qValue, int nq,
                                                                 const KfdbSlot* __restrict__ slots, int nslots,
                                                                 const uint32_t* __restrict__ word, const double* __restrict__ value,
                                                                 KfdbAnswer* __restrict__ out) {
  extern __shared__ uint32_t sq[];
  for (int i = threadIdx.x; i < nq; i += blockDim.x) sq[i] = qWord[i];
  __syncthreads();
  const int lane = lane_id();
  const int wavesPerBlock = blockDim.x >> 6;
  const int stride = gridDim.x * wavesPerBlock;
  for (int s = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); s < nslots; s += stride) {
    const KfdbSlot sl = slots[s];
    int common = 0, first = -1;
    double acc = 0;                                            // `double score = 0;` (:32)
    for (int base = 0; base < sl.count; base += 64) {
      const int i = base + lane;
      bool hit = false;
      int at = 0;
      double term = 0;
      if (i < sl.count) {
        const uint32_t w = word[sl.off + i];
        int lo = 0, hi = nq;                                   // the first query word >= w
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sq[mid] < w) lo = mid + 1; else hi = mid;
        }
        if (lo < nq && sq[lo] == w) {
          hit = true;
          at = lo;
          const double vi = qValue[lo], wi = value[sl.off + i];
          term = fabs(vi - wi) - fabs(vi) - fabs(wi);          // (:41), left to right
        }
      }
      unsigned long long mask = __ballot(hit);
      if (!mask) continue;
      common += __popcll(mask);
      if (first < 0) first = __shfl(at, __ffsll((long long)mask) - 1, 64);
      while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        acc += __shfl(term, src, 64);
        mask &= mask - 1;
      }
    }
    if (lane == 0) {
      KfdbAnswer a;
      a.common = common; a.first = first; a.score = -acc / 2.0;     // (:65): -0.0 when nothing is shared
      out[s] = a;
    }
  }
}

}  // namespace pli
