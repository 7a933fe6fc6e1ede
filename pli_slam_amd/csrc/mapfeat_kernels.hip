// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:300-365) and MapLine::ComputeDistinctiveDescriptors (MapLine.cc:246-317) for a
// batch of features: of the N descriptors that observe a feature, the one whose median distance to all N (itself included) is least.
//
//   D[i][j]   = hamming(d_i, d_j), D[i][i] = 0                          (MapPoint.cc:333-343; MapLine.cc:282-293 stores every pair twice)
//   median_i  = sorted(D[i][0..N))[int(0.5 * (N - 1))]                  (:350-352: the lower median, the diagonal's zero is in the row)
//   BestIdx   = the lowest i with the least median_i                    (:354 tests `median < BestMedian` strictly)
//
// For N = 1 and N = 2 every median is 0 and BestIdx = 0.  The largest distance is 256 (a descriptor and its complement), so a median
// takes 9 bits, and the winner is the minimum of the key median * 4096 + i (i < PLI_DISTINCTIVE_MAX_OBS = 2048).
//
// No row is sorted.  With k = (N - 1) / 2 and cnt(v) = #{j : D[i][j] <= v}, cnt ascends in v and sorted[k] is the smallest v with
// cnt(v) >= k + 1: below it at most k entries are <= v, so sorted[k] > v; at it at least k + 1 are, so sorted[k] <= v.  The values
// lie in [0, 256] (257 of them), so a bisection finds that v in nine steps of N comparisons each.
//
// The groups are independent.  The host sorts them into two size classes (match_capi.hip: pli_distinctive_descriptors): one launch for
// the small class, two for the large one.  Every loop below is bounded by N, by the nine steps or by a list's length, no workgroup
// waits for another, and there are no atomics.
#include "kernels.hpp"
#include "device_prims.hpp"

namespace pli {

namespace {

__device__ __forceinline__ void load_desc(uint64_t d[4], const uint64_t* __restrict__ p) {
  d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = p[3];
}

}  // namespace

// Small class, 1 <= N <= 64: one wave per group, four groups per 256-thread workgroup at a time, the list strided over the waves of
// the grid.  Lane i holds descriptor i; descriptor j reaches all lanes from the wave's LDS stage (one address per wave: a broadcast
// read).  Row i's distances lie in the wave's own LDS slice as u16 [j][lane] (8 KiB), which the bisection then walks.
__global__ __launch_bounds__(DISTINCTIVE_BLOCK) void k_distinctive_wave(const uint8_t* __restrict__ desc, const int* __restrict__ off,
                                                                        const int* __restrict__ list, int nlist, int* __restrict__ best,
                                                                        int* __restrict__ bestMedian, int* __restrict__ rowMedian) {
  __shared__ uint64_t sDesc[DISTINCTIVE_BLOCK / 64][64 * 4];
  __shared__ uint16_t sDist[DISTINCTIVE_BLOCK / 64][64 * 64];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int wavesPerBlock = blockDim.x >> 6;
  const int stride = gridDim.x * wavesPerBlock;
  uint64_t* myDesc = sDesc[wave];
  uint16_t* myDist = sDist[wave];
  for (int g = blockIdx.x * wavesPerBlock + wave; g < nlist; g += stride) {
    const int p = list[g];
    const int base = off[p], n = off[p + 1] - base;               // 1 <= n <= 64 (the host's classes)
    uint64_t di[4] = {0, 0, 0, 0};
    if (lane < n) load_desc(di, reinterpret_cast<const uint64_t*>(desc) + ((size_t)base + lane) * 4);
    wave_lds_sync();                                               // (the previous group's reads of the stage are done)
    myDesc[lane * 4 + 0] = di[0]; myDesc[lane * 4 + 1] = di[1]; myDesc[lane * 4 + 2] = di[2]; myDesc[lane * 4 + 3] = di[3];
    wave_lds_sync();
    for (int j = 0; j < n; ++j) {
      uint64_t dj[4];
      load_desc(dj, myDesc + j * 4);
      myDist[j * 64 + lane] = (uint16_t)hamming256(di, dj);
    }
    const int need = ((n - 1) >> 1) + 1;
    int lo = 0, hi = 256;
    for (int step = 0; step < 9; ++step) {
      const int mid = (lo + hi) >> 1;
      int cnt = 0;
      for (int j = 0; j < n; ++j) cnt += (int)myDist[j * 64 + lane] <= mid ? 1 : 0;     // (a lane reads only what it wrote)
      if (cnt >= need) hi = mid; else lo = mid + 1;
    }
    unsigned long long key = ~0ull;
    if (lane < n) {
      key = (unsigned long long)lo * 4096ull + (unsigned)lane;
      rowMedian[base + lane] = lo;
    }
    key = wave_min_u64(key);
    if (lane == 0) {
      best[p] = (int)(key & 4095ull);
      bestMedian[p] = (int)(key >> 12);
    }
  }
}

// Large class, 64 < N <= PLI_DISTINCTIVE_MAX_OBS.  The rows of a group are independent until the winner is picked, so the host cuts a
// group into chunks of 256 rows (DistinctiveChunk) and a 256-thread workgroup takes one chunk at a time, a row per thread, the chunks
// strided over the grid.  The workgroup stages the whole group's descriptors in LDS (dynamic: 32 bytes times the longest group of the
// launch, 64 KiB at the cap), and descriptor j is read at one LDS address for the whole workgroup (a broadcast).  A thread keeps no
// row of distances (2 * N bytes each would not fit): it recomputes them in every bisection step.  The medians go to row_median;
// k_distinctive_pick, launched behind it on the same stream, takes the winner from there: no workgroup waits for another.
__global__ __launch_bounds__(DISTINCTIVE_BLOCK) void k_distinctive_block(const uint8_t* __restrict__ desc, const int* __restrict__ off,
                                                                         const DistinctiveChunk* __restrict__ chunks, int nchunks,
                                                                         int* __restrict__ rowMedian) {
  extern __shared__ uint64_t sDesc[];                              // n * 4 words
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const DistinctiveChunk ch = chunks[c];
    const int base = off[ch.group], n = off[ch.group + 1] - base;
    const uint64_t* own = reinterpret_cast<const uint64_t*>(desc) + (size_t)base * 4;
    __syncthreads();                                               // (the previous chunk's reads are done)
    for (int w = threadIdx.x; w < n * 4; w += blockDim.x) sDesc[w] = own[w];
    __syncthreads();
    const int i = ch.firstRow + threadIdx.x;
    if (i >= n) continue;                                          // (no barrier below)
    const int need = ((n - 1) >> 1) + 1;
    uint64_t di[4];
    load_desc(di, sDesc + (size_t)i * 4);
    int lo = 0, hi = 256;
    for (int step = 0; step < 9; ++step) {
      const int mid = (lo + hi) >> 1;
      int cnt = 0;
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        uint64_t dj[4];
        load_desc(dj, sDesc + (size_t)j * 4);
        cnt += hamming256(di, dj) <= mid ? 1 : 0;
      }
      if (cnt >= need) hi = mid; else lo = mid + 1;
    }
    rowMedian[base + i] = lo;
  }
}

// The winner of every group of the large class from its rows' medians: one wave per group, the groups strided over the waves of the
// grid, the rows over the lanes.
__global__ __launch_bounds__(DISTINCTIVE_BLOCK) void k_distinctive_pick(const int* __restrict__ off, const int* __restrict__ list, int nlist,
                                                                        const int* __restrict__ rowMedian, int* __restrict__ best,
                                                                        int* __restrict__ bestMedian) {
  const int wavesPerBlock = blockDim.x >> 6;
  for (int g = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); g < nlist; g += gridDim.x * wavesPerBlock) {
    const int p = list[g];
    const int base = off[p], n = off[p + 1] - base;
    unsigned long long key = ~0ull;
    for (int i = lane_id(); i < n; i += 64) {
      const unsigned long long k = (unsigned long long)rowMedian[base + i] * 4096ull + (unsigned)i;
      key = k < key ? k : key;
    }
    key = wave_min_u64(key);
    if (lane_id() == 0) {
      best[p] = (int)(key & 4095ull);
      bestMedian[p] = (int)(key >> 12);
    }
  }
}

}  // namespace pli
