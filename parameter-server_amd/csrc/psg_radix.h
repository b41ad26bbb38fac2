// psg_radix.h — one stable counting pass over a key list, by a digit the
// caller names: the scan and scatter kernels of the LSD radix sort
// (psg_sort.hip, the digit is 8 bits of the key) and of the worker's routing
// pass (psg_route.hip, the digit is the server that owns the key).
//
// One tile of 4096 items per 256-thread block:
//   a histogram kernel of the caller's   counts[digit][tile]
//   k_rs_scan     per digit, exclusive scan over the tiles; digit totals
//   k_rs_scatter  every tile ranks its items stably inside the tile (16 rounds
//                 of 256 items in position order; a wave finds the lanes that
//                 share its digit with kBits ballots), reorders them by digit in
//                 LDS, and writes each digit's run to its global place:
//                 consecutive lanes -> consecutive addresses within a run.
//
// A Digit is a small functor passed by value:
//   static constexpr int kBits        digits are in [0, 1 << kBits), kBits <= 8
//   __device__ void prepare() const   once per block, before the first barrier
//                                     (state it keeps in LDS)
//   __device__ uint32_t operator()(K) the digit of a key
#pragma once
#include "psg_internal.h"

namespace psg {

constexpr int kRsBlock = 256;
constexpr int kRsRounds = 16;
constexpr int kRsTile = kRsBlock * kRsRounds;  // 4096 items per block
constexpr int kRsWaves = kRsBlock / 64;

inline uint64_t rs_tiles(uint64_t n) { return (n + kRsTile - 1) / kRsTile; }

// exclusive scan over 256 lanes of a block (4 waves)
__device__ __forceinline__ uint32_t rs_block_scan(uint32_t v, uint32_t* total, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kRsWaves; ++k) {
    if (k < w) off += wsum[k];
    tot += wsum[k];
  }
  __syncthreads();
  *total = tot;
  return off + x - v;
}

// one block per digit: counts[d][0..ntiles) -> exclusive prefix; dtot[d] = total.
// A template only so that every file that includes this header shares one copy.
template <typename = void>
__global__ __launch_bounds__(kRsBlock) void k_rs_scan(uint32_t* __restrict__ counts, uint64_t ntiles,
                                                      uint32_t* __restrict__ dtot) {
  __shared__ uint32_t wsum[kRsWaves];
  uint32_t* c = counts + (uint64_t)blockIdx.x * ntiles;
  uint32_t carry = 0;
  for (uint64_t b = 0; b < ntiles; b += kRsBlock) {
    const uint64_t i = b + threadIdx.x;
    const uint32_t v = i < ntiles ? c[i] : 0u;
    uint32_t tot;
    const uint32_t ex = rs_block_scan(v, &tot, wsum);
    if (i < ntiles) c[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) dtot[blockIdx.x] = carry;
}

template <typename K, bool IOTA, typename Digit>
__global__ __launch_bounds__(kRsBlock) void k_rs_scatter(const K* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                         K* __restrict__ kout, uint32_t* __restrict__ vout,
                                                         uint64_t n, Digit digit,
                                                         const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ dtot, uint64_t ntiles) {
  constexpr int NB = 1 << Digit::kBits;  // digits
  static_assert(NB <= kRsBlock, "a lane per digit");
  __shared__ K sK[kRsTile];
  __shared__ uint32_t sV[kRsTile];
  __shared__ uint32_t gbase[NB], lstart[NB], running[NB];
  __shared__ uint32_t wcnt[kRsWaves][NB];
  __shared__ uint32_t wsum[kRsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool own = NB >= kRsBlock || tid < NB;  // this lane keeps digit tid's counters
  const uint64_t tile = blockIdx.x, t0 = tile * kRsTile;
  digit.prepare();
  {
    // global start of digit tid = sum of the smaller digits' totals; this
    // tile's place in it = the scanned count of the earlier tiles
    uint32_t tot;
    const uint32_t ds = rs_block_scan(own ? dtot[tid] : 0u, &tot, wsum);
    if (own) {
      gbase[tid] = ds + counts[(uint64_t)tid * ntiles + tile];
      running[tid] = 0;
#pragma unroll
      for (int w = 0; w < kRsWaves; ++w) wcnt[w][tid] = 0;
    }
  }
  K key[kRsRounds];
  uint32_t val[kRsRounds], rank[kRsRounds];
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kRsBlock + tid;
    key[r] = i < n ? kin[i] : (K)0;
    val[r] = IOTA ? (uint32_t)i : (i < n ? vin[i] : 0u);
  }
  __syncthreads();
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // 16 rounds in position order: round r holds items t0 + r*256 + tid, so
  // (round, wave, lane) order is position order and every rank is stable
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kRsBlock + tid;
    const bool valid = i < n;
    const uint32_t d = digit(key[r]);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < Digit::kBits; ++b) {
      const uint64_t bb = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? bb : ~bb;
    }
    const uint32_t in_wave = (uint32_t)__popcll(peers & lt);
    if (valid && in_wave == 0) wcnt[wv][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t before = running[d];
      for (int w = 0; w < wv; ++w) before += wcnt[w][d];
      rank[r] = before + in_wave;
    }
    __syncthreads();
    if (own) {
      uint32_t add = 0;
#pragma unroll
      for (int w = 0; w < kRsWaves; ++w) {
        add += wcnt[w][tid];
        wcnt[w][tid] = 0;
      }
      running[tid] += add;
    }
    __syncthreads();
  }
  {
    uint32_t tot;
    const uint32_t ls = rs_block_scan(own ? running[tid] : 0u, &tot, wsum);
    if (own) lstart[tid] = ls;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kRsBlock + tid;
    if (i < n) {
      const uint32_t p = lstart[digit(key[r])] + rank[r];
      sK[p] = key[r];
      sV[p] = val[r];
    }
  }
  __syncthreads();
  const uint64_t tn = n - t0 < (uint64_t)kRsTile ? n - t0 : (uint64_t)kRsTile;
  for (uint32_t j = tid; j < tn; j += kRsBlock) {
    const K k = sK[j];
    const uint32_t d = digit(k);
    const uint64_t g = (uint64_t)gbase[d] + (j - lstart[d]);
    kout[g] = k;
    vout[g] = sV[j];
  }
}

}  // namespace psg
