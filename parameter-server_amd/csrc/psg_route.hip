// psg_route.hip — worker-side routing of a key list in any order, with repeats,
// to the servers that own its keys, and the row copies that go with it.
//
//   psg_route         the stable partition of keys[n] by owning server: what
//                     DefaultSlicer's lower_bounds (src/ps/KVApp.h:515-574)
//                     cannot give for a list that is not sorted
//   psg_rows_gather   dst row r = src row perm[r]   (values into routed order)
//   psg_rows_scatter  dst row perm[r] = src row r   (replies back to the caller's)
//
// Routing is ONE stable counting pass whose digit is the owner (psg_radix.h, the
// machinery of psg_sort.hip's passes):
//   k_route_hist  every key read once; its owner by a 6-step search over the
//                 range ends in LDS; counts[owner][tile]; a flag when a key lies
//                 outside the ranges, another when an owner is lower than its
//                 predecessor's
//   k_rs_scan     per owner, exclusive scan over the tiles; owner totals
//   (host)        totals and flags read after one synchronisation: key_pos; a
//                 list whose owners never decrease is already partitioned and
//                 is left where it is
//   k_rs_scatter  rank inside the tile by wave ballots and per-wave counts in
//                 LDS, so arrival order is kept; writes routed_keys and perm
// Bytes per key: 8 read for a list already partitioned, else 8 + 8 read and
// 8 + 4 written.
//
// The two row copies walk the rows as one flat stream of units, as k_rows_walk
// (psg_rows.hip) does, kUnroll loads a lane in flight.  perm is a permutation:
// every row has one writer, no atomics.  Traffic: perm 4 B + 2 * row_bytes a row.
//
// Bags across servers (the pooled lookup and update of psg_rows.hip, sharded):
//   psg_route_bags    every server's share of every bag of a routed list, as
//                     the nb + 1 offsets of that server's stretch
//   psg_pool_reduce   the servers' pooled partial rows added in rank order
//   k_bags_check      the three rules of an offsets array (k_offsets_check's,
//                     psg_rows.hip), in front of everything else that reads it
//   k_bags_split      one lane per (server, offset): a lower bound over the
//                     server's ascending stretch of perm, or a clamp when the
//                     list was left in place; writes nothing it was refused
//   k_pool_reduce     one lane per 16-B vector (or element): k loads, k adds
//                     from +0 in the accumulator's type, one store; no atomics
// A mean over a sharded bag (no server sees a bag's whole length):
//   psg_pool_reduce_mean  the fold of the servers' SUM partials, divided once by
//                         the bag's length from the caller's offsets
//   psg_pool_scale_mean   the bags' gradient rows divided once, into the pooled
//                         frame every server then takes as a plain sum's
//   k_pool_reduce_mean, k_pool_scale_mean   one lane per 16-B vector when a row
//                     is whole vectors (no vector straddles two bags), else per
//                     element; the two offsets words of the bag beside the loads
#include <algorithm>
#include <map>

#include "psg_radix.h"

namespace psg {

namespace {

constexpr int kMaxServers = PSG_ROUTE_MAX_SERVERS;
constexpr uint64_t kMaxRouted = 0xfffffffeull;
constexpr uint32_t kMaxRowBytes = 4096 * 8;

struct Ends {
  uint64_t v[kMaxServers];  // ends[0 .. ns-1) (the last end bounds no owner)
};

// The owner of a key as a digit: the number of range ends at or below it, at
// most ns - 1 (a key at or above the last end is rejected by k_route_hist; here
// it only has to stay inside the counters).
struct OwnerDigit {
  static constexpr int kBits = 6;
  static_assert((1 << kBits) == kMaxServers, "a digit per server");
  Ends e;
  uint32_t nsm1;  // ns - 1
  static __device__ __forceinline__ uint64_t* lds() {
    __shared__ uint64_t s_ends[kMaxServers];
    return s_ends;
  }
  __device__ __forceinline__ void prepare() const {
    if (threadIdx.x < (unsigned)kMaxServers) lds()[threadIdx.x] = e.v[threadIdx.x];
  }
  __device__ __forceinline__ uint32_t operator()(uint64_t k) const {
    const uint64_t* ends = lds();
    uint32_t o = 0;
#pragma unroll
    for (uint32_t step = kMaxServers / 2; step; step >>= 1)
      if (o + step <= nsm1 && ends[o + step - 1] <= k) o += step;
    return o;
  }
};

enum { F_RANGE = 0, F_ORDER = 1, kNFlags = 2 };

// Pass 1.  counts[owner][tile]; flags[F_RANGE] when a key lies outside [lo, hi),
// flags[F_ORDER] when some key's owner is lower than its predecessor's.  A wave
// finds the lanes that share an owner with kBits ballots (as k_rs_scatter does)
// and their first lane adds their number: a list that goes to two servers would
// otherwise put 256 LDS atomics on two words.
__global__ __launch_bounds__(kRsBlock) void k_route_hist(const uint64_t* __restrict__ keys, uint64_t n,
                                                         OwnerDigit digit, uint64_t lo, uint64_t hi,
                                                         uint32_t* __restrict__ counts, uint64_t ntiles,
                                                         int* __restrict__ flags) {
  __shared__ uint32_t h[kMaxServers];
  const int tid = threadIdx.x, lane = tid & 63;
  digit.prepare();
  if (tid < kMaxServers) h[tid] = 0;
  __syncthreads();
  const uint64_t t0 = (uint64_t)blockIdx.x * kRsTile;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  bool bad = false, desc = false;
#pragma unroll 4
  for (int r = 0; r < kRsRounds; ++r) {
    const uint64_t i = t0 + (uint64_t)r * kRsBlock + tid;
    const bool valid = i < n;
    const uint64_t k = valid ? keys[i] : 0;
    const uint32_t o = digit(k);
    bad |= valid && (k < lo || k >= hi);
    // the predecessor's owner: the lane below, or for a wave's first lane the
    // key before it (a line the wave below has just read)
    uint32_t prev = __shfl_up(o, 1, 64);
    if (lane == 0) prev = (valid && i > 0) ? digit(keys[i - 1]) : o;
    desc |= valid && o < prev;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < OwnerDigit::kBits; ++b) {
      const uint64_t bb = __ballot((o >> b) & 1u);
      peers &= ((o >> b) & 1u) ? bb : ~bb;
    }
    if (valid && (peers & lt) == 0) atomicAdd(&h[o], (uint32_t)__popcll(peers));
  }
  if (__ballot(bad) && lane == 0) flags[F_RANGE] = 1;
  if (__ballot(desc) && lane == 0) flags[F_ORDER] = 1;
  __syncthreads();
  if (tid < kMaxServers) counts[(uint64_t)tid * ntiles + blockIdx.x] = h[tid];
}

// dst row r = src row perm[r] (GATHER), or dst row perm[r] = src row r, for
// r < n; rows of upr units of type U.  A position of perm outside [0, n) is
// skipped: no row there to read or write.
template <typename U, bool GATHER>
__global__ __launch_bounds__(256) void k_rows_permute(U* __restrict__ dst, const U* __restrict__ src,
                                                      const uint32_t* __restrict__ perm, uint64_t n, uint32_t upr,
                                                      uint32_t rpt) {
  constexpr int UN = kUnroll;
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UN * kBlock) {
      uint64_t so[UN] = {}, to[UN] = {};
      bool ok[UN];
      U v[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t r = i0 + w.r;
          const uint64_t p = perm[r];
          ok[k] = p < n;
          so[k] = (GATHER ? p : r) * upr + w.c;
          to[k] = (GATHER ? r : p) * upr + w.c;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) v[k] = src[so[k]];
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) dst[to[k]] = v[k];
    }
  }
}

template <typename U, bool GATHER>
int launch_permute(void* dst, const void* src, const uint32_t* perm, uint64_t n, uint32_t upr, hipStream_t st) {
  const uint32_t rpt = rows_per_tile(upr);
  uint64_t blocks = (n + rpt - 1) / rpt;
  blocks = std::min<uint64_t>(blocks, (uint64_t)max_stream_blocks());
  k_rows_permute<U, GATHER><<<(unsigned)blocks, kBlock, 0, st>>>((U*)dst, (const U*)src, perm, n, upr, rpt);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// rows move as raw bytes, in the widest unit the row length and both pointers allow
template <bool GATHER>
int permute_rows(const char* name, void* dst, const void* src, const uint32_t* perm, uint64_t n, uint64_t row_bytes,
                 hipStream_t st) {
  PSG_REQUIRE(row_bytes >= 1 && row_bytes <= kMaxRowBytes, PSG_ERR_INVALID, "%s: row_bytes %llu outside [1, %u]", name,
              (unsigned long long)row_bytes, kMaxRowBytes);
  PSG_REQUIRE(n <= kMaxRouted, PSG_ERR_INVALID, "%s: %llu rows, more than 2^32-2", name, (unsigned long long)n);
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(dst && src, PSG_ERR_INVALID, "%s: null rows", name);
  PSG_REQUIRE(perm, PSG_ERR_INVALID, "%s: null perm", name);
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | (uintptr_t)row_bytes;
  const uint32_t rb = (uint32_t)row_bytes;
  if (a % 16 == 0) return launch_permute<u32x4, GATHER>(dst, src, perm, n, rb / 16, st);
  if (a % 8 == 0) return launch_permute<uint64_t, GATHER>(dst, src, perm, n, rb / 8, st);
  if (a % 4 == 0) return launch_permute<uint32_t, GATHER>(dst, src, perm, n, rb / 4, st);
  if (a % 2 == 0) return launch_permute<uint16_t, GATHER>(dst, src, perm, n, rb / 2, st);
  return launch_permute<uint8_t, GATHER>(dst, src, perm, n, rb, st);
}

// Per-thread, per-GPU scratch of the route, as the slicer's (psg_slice.hip):
// the counters in HBM, grown on demand, and a pinned mirror of their tail, so a
// steady caller allocates nothing.  Layout: counts[kMaxServers][ntiles], then
// the kMaxServers owner totals, then the flags.
constexpr int kTail = kMaxServers + kNFlags;
struct RouteScratch {
  uint32_t* counts = nullptr;
  uint64_t cap = 0;  // words
  uint32_t* tail_host = nullptr;
};
thread_local std::map<int, RouteScratch> t_route_scratch;

int get_route_scratch(uint64_t words, RouteScratch** out) {
  int dev = 0;
  PSG_HIP(hipGetDevice(&dev));
  RouteScratch& s = t_route_scratch[dev];
  if (!s.tail_host) PSG_HIP(hipHostMalloc((void**)&s.tail_host, kTail * sizeof(uint32_t), hipHostMallocDefault));
  if (s.cap < words) {
    if (s.counts) PSG_HIP(hipFree(s.counts));
    s.counts = nullptr;
    s.cap = 0;
    const uint64_t cap = std::max<uint64_t>(words * 2, 1 << 16);
    PSG_HIP(hipMalloc((void**)&s.counts, cap * sizeof(uint32_t)));
    s.cap = cap;
  }
  *out = &s;
  return PSG_OK;
}

// ---- bags across servers ------------------------------------------------------
// The three rules of a bag list (k_offsets_check, psg_rows.hip): offsets[0] == 0,
// no offset above its successor, offsets[nb] == n.  8 B read per bag.  A broken
// rule raises *gate (a device word k_bags_split reads) and *flag_host (pinned
// host memory, read by the host after the one synchronisation).
__global__ __launch_bounds__(256) void k_bags_check(const uint64_t* __restrict__ offsets, uint64_t nb, uint64_t n,
                                                    int* __restrict__ gate, int* __restrict__ flag_host) {
  bool bad = false;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * kBlock) {
    const uint64_t o = offsets[b];
    if (b == 0 && o != 0) bad = true;
    if (b == nb ? o != n : offsets[b + 1] < o) bad = true;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) {
    *gate = 1;
    *flag_host = 1;
  }
}

struct KeyPos {
  uint64_t v[kMaxServers + 1];  // key_pos[0 .. ns]
};

// so[s][b] = #{ r in [key_pos[s], key_pos[s+1]) : perm[r] < offsets[b] }, one lane
// per (s, b), b in [0, nb].  Server s's stretch of perm ascends (the partition is
// stable), so the count is a lower bound: at most 32 dependent 4-B probes, over
// lines the lanes of neighbouring bags share.  IDENT: the list was left in
// place, perm[r] == r, and the count is a clamp.  Launched behind k_bags_check
// without the host in between: a launch that finds *gate raised writes nothing.
// Every read of perm lies inside [0, key_pos[ns]) whatever the offsets hold.
template <bool IDENT>
__global__ __launch_bounds__(256) void k_bags_split(const uint64_t* __restrict__ offsets, uint64_t nb,
                                                    const uint32_t* __restrict__ perm, KeyPos kp, uint32_t ns,
                                                    uint64_t* __restrict__ so, const int* __restrict__ gate) {
  __shared__ uint64_t s_kp[kMaxServers + 1];
  if (threadIdx.x <= (unsigned)kMaxServers) s_kp[threadIdx.x] = kp.v[threadIdx.x];
  __syncthreads();
  if (*gate) return;
  const uint64_t per = nb + 1, total = (uint64_t)ns * per;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t s = i / per;
    const uint64_t o = offsets[i - s * per];
    const uint64_t lo = s_kp[s], hi = s_kp[s + 1];
    uint64_t a = lo, b = hi;
    if (IDENT) {
      a = o < lo ? lo : o > hi ? hi : o;
    } else {
      while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (perm[mid] < o) a = mid + 1;
        else b = mid;
      }
    }
    so[i] = a - lo;
  }
}

// Scratch of psg_route_bags, per thread and GPU as the route's: the gate word in
// HBM and the pinned flag word.
struct BagScratch {
  int* gate = nullptr;
  int* flag_host = nullptr;
  int* flag_dev = nullptr;  // device view of flag_host
};
thread_local std::map<int, BagScratch> t_bag_scratch;

int get_bag_scratch(BagScratch** out) {
  int dev = 0;
  PSG_HIP(hipGetDevice(&dev));
  BagScratch& s = t_bag_scratch[dev];
  if (!s.flag_host) {
    PSG_HIP(hipHostMalloc((void**)&s.flag_host, sizeof(int), hipHostMallocMapped));
    PSG_HIP(hipHostGetDevicePointer((void**)&s.flag_dev, s.flag_host, 0));
  }
  if (!s.gate) PSG_HIP(hipMalloc((void**)&s.gate, sizeof(int)));
  *out = &s;
  return PSG_OK;
}

// out unit i = round(((+0 + p[0][i]) + p[1][i]) + ... + p[k-1][i]), the adds in
// the accumulator's type (PoolAcc): the fold of the servers' pooled partials in
// rank order.  One lane per unit, grid-strided; four loads of a unit in flight,
// then their four adds in order.  The pointers ride in the kernel's arguments
// and are indexed by a wave-uniform s.  (k + 1) * sizeof(U) bytes a unit.
struct Partials {
  const void* p[kMaxServers];
};

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void k_pool_reduce(typename PoolAcc<DT, VEC>::U* __restrict__ out, Partials ps, int k,
                                                     uint64_t units) {
  typedef PoolAcc<DT, VEC> P;
  typedef typename P::U U;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < units; i += (uint64_t)gridDim.x * kBlock) {
    typename P::A acc{};
    int s = 0;
    for (; s + 4 <= k; s += 4) {
      const U v0 = ((const U*)ps.p[s])[i], v1 = ((const U*)ps.p[s + 1])[i];
      const U v2 = ((const U*)ps.p[s + 2])[i], v3 = ((const U*)ps.p[s + 3])[i];
      acc = P::add(acc, v0);
      acc = P::add(acc, v1);
      acc = P::add(acc, v2);
      acc = P::add(acc, v3);
    }
    for (; s < k; ++s) acc = P::add(acc, ((const U*)ps.p[s])[i]);
    out[i] = P::round(acc);
  }
}

// ---- a mean over a sharded bag --------------------------------------------------
// A lane's grid-strided walk over nb rows of upr units: unit i is column c of
// row b.  The first unit of a lane lies below 2^19 (the grid's cap), so the one
// division is a 32-bit one; a step of the whole grid is (dr, dc), cut on the host.
struct BagWalk {
  uint64_t b;
  uint32_t c, upr, dc;
  uint64_t dr;
  __device__ __forceinline__ BagWalk(uint32_t i0, uint32_t units_per_row, uint64_t step_rows, uint32_t step_cols)
      : b(i0 / units_per_row), c(i0 - (i0 / units_per_row) * units_per_row), upr(units_per_row), dc(step_cols),
        dr(step_rows) {}
  __device__ __forceinline__ void next() {
    b += dr;
    c += dc;
    if (c >= upr) {
      c -= upr;
      ++b;
    }
  }
};

// out unit i = round(fold(i) / L_b), fold as k_pool_reduce's, b the bag (row) of
// unit i, L_b = offsets[b+1] - offsets[b] read as 32 bits: the mean of a bag
// whose ids lie on several servers, from their SUM partials.  One correctly
// rounded division in the accumulator's type (PoolAcc::over, as k_rows_pool); an
// empty bag stores +0 and divides nothing.  A unit lies inside one row (VEC only
// when a row is whole vectors), so a lane needs one length.  The two offsets
// words are loaded with the partials, ahead of the adds.  (k + 1) * sizeof(U)
// bytes a unit and 16 B a bag, which the lanes of a row share.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void k_pool_reduce_mean(typename PoolAcc<DT, VEC>::U* __restrict__ out, Partials ps,
                                                          int k, const uint64_t* __restrict__ offsets, uint64_t units,
                                                          uint32_t upr, uint64_t dr, uint32_t dc) {
  typedef PoolAcc<DT, VEC> P;
  typedef typename P::U U;
  const uint32_t i0 = blockIdx.x * kBlock + threadIdx.x;
  BagWalk w(i0, upr, dr, dc);
  for (uint64_t i = i0; i < units; i += (uint64_t)gridDim.x * kBlock, w.next()) {
    const uint64_t o0 = offsets[w.b], o1 = offsets[w.b + 1];
    typename P::A acc{};
    int s = 0;
    for (; s + 4 <= k; s += 4) {
      const U v0 = ((const U*)ps.p[s])[i], v1 = ((const U*)ps.p[s + 1])[i];
      const U v2 = ((const U*)ps.p[s + 2])[i], v3 = ((const U*)ps.p[s + 3])[i];
      acc = P::add(acc, v0);
      acc = P::add(acc, v1);
      acc = P::add(acc, v2);
      acc = P::add(acc, v3);
    }
    for (; s < k; ++s) acc = P::add(acc, ((const U*)ps.p[s])[i]);
    const uint32_t len = (uint32_t)(o1 - o0);
    if (len) acc = P::over(acc, len);
    else acc = typename P::A{};
    out[i] = P::round(acc);
  }
}

// dst unit i = grads unit i / (float)L_b: the gradient rows of mean bags, divided
// once for every server (k_pool_reduce_mean's walk and lengths).  An empty bag's
// row is +0 and its gradient row is not read.  8 B a float and 16 B a bag.
template <bool VEC>
__global__ __launch_bounds__(256) void k_pool_scale_mean(typename PoolAcc<PSG_F32, VEC>::U* __restrict__ dst,
                                                         const typename PoolAcc<PSG_F32, VEC>::U* __restrict__ grads,
                                                         const uint64_t* __restrict__ offsets, uint64_t units,
                                                         uint32_t upr, uint64_t dr, uint32_t dc) {
  typedef PoolAcc<PSG_F32, VEC> P;
  const uint32_t i0 = blockIdx.x * kBlock + threadIdx.x;
  BagWalk w(i0, upr, dr, dc);
  for (uint64_t i = i0; i < units; i += (uint64_t)gridDim.x * kBlock, w.next()) {
    const uint32_t len = (uint32_t)(offsets[w.b + 1] - offsets[w.b]);
    typename P::A acc{};
    if (len) acc = P::over(P::widen(grads[i]), len);
    dst[i] = P::round(acc);
  }
}

// the grid of a walk over nb rows of upr units, and its step cut into (dr, dc)
struct BagGrid {
  uint64_t units, dr;
  uint32_t upr, dc;
  unsigned blocks;
  BagGrid(uint64_t nb, uint32_t units_per_row) : units(nb * units_per_row), upr(units_per_row) {
    blocks = (unsigned)std::min<uint64_t>((units + kBlock - 1) / kBlock, (uint64_t)max_stream_blocks());
    const uint64_t step = (uint64_t)blocks * kBlock;
    dr = step / upr;
    dc = (uint32_t)(step - dr * upr);
  }
};

template <int DT>
int launch_pool_reduce_mean(void* out, const Partials& ps, int k, const uint64_t* offsets, uint64_t nb, uint32_t width,
                            bool vec, hipStream_t st) {
  const BagGrid g(nb, vec ? width / Elem<DT>::kVec : width);
  if (vec)
    k_pool_reduce_mean<DT, true><<<g.blocks, kBlock, 0, st>>>((typename PoolAcc<DT, true>::U*)out, ps, k, offsets,
                                                              g.units, g.upr, g.dr, g.dc);
  else
    k_pool_reduce_mean<DT, false><<<g.blocks, kBlock, 0, st>>>((typename PoolAcc<DT, false>::U*)out, ps, k, offsets,
                                                               g.units, g.upr, g.dr, g.dc);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// [p, p + bytes) and [q, q + bytes) share no byte
inline bool apart(uintptr_t p, uintptr_t q, unsigned __int128 bytes) { return p >= q ? p - q >= bytes : q - p >= bytes; }

template <int DT>
int launch_pool_reduce(void* out, const Partials& ps, int k, uint64_t count, bool vec, hipStream_t st) {
  const uint64_t units = vec ? count / Elem<DT>::kVec : count;
  const uint64_t blocks = std::min<uint64_t>((units + kBlock - 1) / kBlock, (uint64_t)max_stream_blocks());
  if (vec)
    k_pool_reduce<DT, true><<<(unsigned)blocks, kBlock, 0, st>>>((typename PoolAcc<DT, true>::U*)out, ps, k, units);
  else
    k_pool_reduce<DT, false><<<(unsigned)blocks, kBlock, 0, st>>>((typename PoolAcc<DT, false>::U*)out, ps, k, units);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

}  // namespace

}  // namespace psg

using namespace psg;

extern "C" {

int psg_route(const uint64_t* keys, uint64_t n, int num_servers, const uint64_t* begins_host,
              const uint64_t* ends_host, uint64_t* routed_keys, uint32_t* perm, uint64_t* key_pos_host,
              int* identity_host, psg_stream stream) {
  PSG_REQUIRE(num_servers > 0 && num_servers <= kMaxServers, PSG_ERR_INVALID, "psg_route: %d servers outside [1, %d]",
              num_servers, kMaxServers);
  PSG_REQUIRE(begins_host && ends_host && key_pos_host && identity_host, PSG_ERR_INVALID,
              "psg_route: null ranges or outputs");
  for (int i = 0; i < num_servers; ++i) {
    PSG_REQUIRE(begins_host[i] <= ends_host[i], PSG_ERR_INVALID, "psg_route: range %d ends before it begins", i);
    PSG_REQUIRE(i == 0 || ends_host[i - 1] == begins_host[i], PSG_ERR_INVALID,
                "psg_route: ranges %d and %d are not adjacent (CHECK_EQ, KVApp.h:531)", i - 1, i);
  }
  PSG_REQUIRE(n <= kMaxRouted, PSG_ERR_INVALID, "psg_route: %llu keys, more than 2^32-2", (unsigned long long)n);
  if (n == 0) {
    for (int i = 0; i <= num_servers; ++i) key_pos_host[i] = 0;
    *identity_host = 1;
    return PSG_OK;
  }
  PSG_REQUIRE(keys, PSG_ERR_INVALID, "psg_route: null keys");
  PSG_REQUIRE(routed_keys && perm, PSG_ERR_INVALID, "psg_route: null routed_keys or perm");
  hipStream_t st = (hipStream_t)stream;
  const uint64_t ntiles = rs_tiles(n);
  RouteScratch* sc = nullptr;
  PSG_TRY(get_route_scratch(kMaxServers * ntiles + kTail, &sc));
  uint32_t* counts = sc->counts;
  uint32_t* dtot = counts + kMaxServers * ntiles;
  int* flags = (int*)(dtot + kMaxServers);
  OwnerDigit digit;
  for (int i = 0; i < kMaxServers; ++i) digit.e.v[i] = i < num_servers - 1 ? ends_host[i] : UINT64_MAX;
  digit.nsm1 = (uint32_t)(num_servers - 1);
  PSG_HIP(hipMemsetAsync(flags, 0, kNFlags * sizeof(int), st));
  k_route_hist<<<(unsigned)ntiles, kRsBlock, 0, st>>>(keys, n, digit, begins_host[0], ends_host[num_servers - 1],
                                                      counts, ntiles, flags);
  k_rs_scan<><<<kMaxServers, kRsBlock, 0, st>>>(counts, ntiles, dtot);
  PSG_HIP(hipGetLastError());
  PSG_HIP(hipMemcpyAsync(sc->tail_host, dtot, kTail * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PSG_HIP(hipStreamSynchronize(st));
  const uint32_t* tail = sc->tail_host;
  if (tail[kMaxServers + F_RANGE]) {
    set_error("psg_route: a key lies outside the server ranges [%llu, %llu) (KVApp.h:544)",
              (unsigned long long)begins_host[0], (unsigned long long)ends_host[num_servers - 1]);
    return PSG_ERR_RANGE;
  }
  key_pos_host[0] = 0;
  for (int i = 0; i < num_servers; ++i) key_pos_host[i + 1] = key_pos_host[i] + tail[i];
  *identity_host = tail[kMaxServers + F_ORDER] ? 0 : 1;
  if (*identity_host) return PSG_OK;
  k_rs_scatter<uint64_t, true><<<(unsigned)ntiles, kRsBlock, 0, st>>>(keys, nullptr, routed_keys, perm, n, digit, counts,
                                                                     dtot, ntiles);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

int psg_rows_gather(void* dst, const void* src, const uint32_t* perm, uint64_t n, uint64_t row_bytes,
                    psg_stream stream) {
  return permute_rows<true>("psg_rows_gather", dst, src, perm, n, row_bytes, (hipStream_t)stream);
}

int psg_rows_scatter(void* dst, const void* src, const uint32_t* perm, uint64_t n, uint64_t row_bytes,
                     psg_stream stream) {
  return permute_rows<false>("psg_rows_scatter", dst, src, perm, n, row_bytes, (hipStream_t)stream);
}

int psg_route_bags(const uint64_t* offsets, uint64_t nb, const uint32_t* perm, uint64_t n, int num_servers,
                   const uint64_t* key_pos_host, uint64_t* server_offsets, psg_stream stream) {
  PSG_REQUIRE(offsets || nb == 0, PSG_ERR_INVALID, "psg_route_bags: null offsets");
  PSG_REQUIRE(server_offsets || nb == 0, PSG_ERR_INVALID, "psg_route_bags: null server_offsets");
  PSG_REQUIRE(key_pos_host, PSG_ERR_INVALID, "psg_route_bags: null key_pos");
  PSG_REQUIRE(num_servers > 0 && num_servers <= kMaxServers, PSG_ERR_INVALID,
              "psg_route_bags: %d servers outside [1, %d]", num_servers, kMaxServers);
  PSG_REQUIRE(key_pos_host[0] == 0 && key_pos_host[num_servers] == n, PSG_ERR_INVALID,
              "psg_route_bags: key_pos does not run from 0 to n = %llu", (unsigned long long)n);
  for (int s = 0; s < num_servers; ++s)
    PSG_REQUIRE(key_pos_host[s] <= key_pos_host[s + 1], PSG_ERR_INVALID, "psg_route_bags: key_pos decreases at server %d",
                s);
  PSG_REQUIRE(n <= kMaxRouted && nb <= kMaxRouted, PSG_ERR_RANGE, "psg_route_bags: %llu keys in %llu bags, more than 2^32-2",
              (unsigned long long)n, (unsigned long long)nb);
  if (nb == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  BagScratch* sc = nullptr;
  PSG_TRY(get_bag_scratch(&sc));
  KeyPos kp;
  for (int s = 0; s <= kMaxServers; ++s) kp.v[s] = key_pos_host[s <= num_servers ? s : num_servers];
  *sc->flag_host = 0;
  PSG_HIP(hipMemsetAsync(sc->gate, 0, sizeof(int), st));
  const uint64_t cap = (uint64_t)max_stream_blocks();
  k_bags_check<<<(unsigned)std::min<uint64_t>((nb + kBlock) / kBlock, cap), kBlock, 0, st>>>(offsets, nb, n, sc->gate,
                                                                                            sc->flag_dev);
  const uint64_t total = (uint64_t)num_servers * (nb + 1);
  const unsigned blocks = (unsigned)std::min<uint64_t>((total + kBlock - 1) / kBlock, cap);
  if (perm)
    k_bags_split<false><<<blocks, kBlock, 0, st>>>(offsets, nb, perm, kp, (uint32_t)num_servers, server_offsets, sc->gate);
  else
    k_bags_split<true><<<blocks, kBlock, 0, st>>>(offsets, nb, nullptr, kp, (uint32_t)num_servers, server_offsets,
                                                  sc->gate);
  PSG_HIP(hipGetLastError());
  PSG_HIP(hipStreamSynchronize(st));
  PSG_REQUIRE(!*sc->flag_host, PSG_ERR_INVALID,
              "psg_route_bags: offsets must start at 0, never decrease and end at n = %llu", (unsigned long long)n);
  return PSG_OK;
}

int psg_pool_reduce(void* out, const void* const* partials_host, int k, uint64_t count, int dtype, psg_stream stream) {
  PSG_REQUIRE(k > 0 && k <= kMaxServers, PSG_ERR_INVALID, "psg_pool_reduce: %d partials outside [1, %d]", k, kMaxServers);
  const uint64_t es = (uint64_t)dtype_size(dtype);
  PSG_REQUIRE(es, PSG_ERR_INVALID, "psg_pool_reduce: unknown dtype %d", dtype);
  PSG_REQUIRE(count <= UINT64_MAX / es, PSG_ERR_RANGE, "psg_pool_reduce: %llu elements overflow a byte count",
              (unsigned long long)count);
  if (count == 0) return PSG_OK;
  PSG_REQUIRE(out && partials_host, PSG_ERR_INVALID, "psg_pool_reduce: null out or partials");
  const uint64_t bytes = count * es;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out);
  uintptr_t a = o | (uintptr_t)bytes;
  Partials ps;
  for (int s = 0; s < kMaxServers; ++s) {
    ps.p[s] = s < k ? partials_host[s] : nullptr;
    if (s >= k) continue;
    const uintptr_t p = reinterpret_cast<uintptr_t>(ps.p[s]);
    PSG_REQUIRE(p, PSG_ERR_INVALID, "psg_pool_reduce: partial %d is null", s);
    PSG_REQUIRE(p >= o ? p - o >= bytes : o - p >= bytes, PSG_ERR_INVALID, "psg_pool_reduce: out overlaps partial %d", s);
    a |= p;
  }
  PSG_REQUIRE(a % es == 0, PSG_ERR_INVALID, "psg_pool_reduce: a pointer is not aligned to its %llu-byte elements",
              (unsigned long long)es);
  const bool vec = a % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case PSG_F32: return launch_pool_reduce<PSG_F32>(out, ps, k, count, vec, st);
    case PSG_F64: return launch_pool_reduce<PSG_F64>(out, ps, k, count, vec, st);
    case PSG_F16: return launch_pool_reduce<PSG_F16>(out, ps, k, count, vec, st);
    default: return launch_pool_reduce<PSG_BF16>(out, ps, k, count, vec, st);
  }
}

int psg_pool_reduce_mean(void* out, const void* const* partials_host, int k, const uint64_t* offsets, uint64_t nb,
                         uint32_t width, int dtype, psg_stream stream) {
  PSG_REQUIRE(k > 0 && k <= kMaxServers, PSG_ERR_INVALID, "psg_pool_reduce_mean: %d partials outside [1, %d]", k,
              kMaxServers);
  const uint64_t es = (uint64_t)dtype_size(dtype);
  PSG_REQUIRE(es, PSG_ERR_INVALID, "psg_pool_reduce_mean: unknown dtype %d", dtype);
  PSG_REQUIRE(width >= 1 && width <= 4096, PSG_ERR_INVALID, "psg_pool_reduce_mean: width %u outside [1, 4096]", width);
  Partials ps;
  for (int s = 0; s < kMaxServers; ++s) ps.p[s] = nullptr;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out);
  uintptr_t a = o;
  if (nb) {
    PSG_REQUIRE(out && partials_host, PSG_ERR_INVALID, "psg_pool_reduce_mean: null out or partials");
    PSG_REQUIRE(offsets, PSG_ERR_INVALID, "psg_pool_reduce_mean: null offsets");
    for (int s = 0; s < k; ++s) {
      ps.p[s] = partials_host[s];
      PSG_REQUIRE(ps.p[s], PSG_ERR_INVALID, "psg_pool_reduce_mean: partial %d is null", s);
      a |= reinterpret_cast<uintptr_t>(ps.p[s]);
    }
    PSG_REQUIRE(a % es == 0, PSG_ERR_INVALID, "psg_pool_reduce_mean: a pointer is not aligned to its %llu-byte elements",
                (unsigned long long)es);
    PSG_REQUIRE(reinterpret_cast<uintptr_t>(offsets) % 8 == 0, PSG_ERR_INVALID,
                "psg_pool_reduce_mean: offsets are not aligned to 8 bytes");
    const unsigned __int128 bytes = (unsigned __int128)nb * width * es;
    for (int s = 0; s < k; ++s)
      PSG_REQUIRE(apart(reinterpret_cast<uintptr_t>(ps.p[s]), o, bytes), PSG_ERR_INVALID,
                  "psg_pool_reduce_mean: out overlaps partial %d", s);
  }
  PSG_REQUIRE(nb <= kMaxRouted, PSG_ERR_RANGE, "psg_pool_reduce_mean: %llu bags, more than 2^32-2", (unsigned long long)nb);
  if (nb == 0) return PSG_OK;
  // a 16-B vector per lane only when it cannot straddle two bags
  const bool vec = (width * es) % 16 == 0 && a % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case PSG_F32: return launch_pool_reduce_mean<PSG_F32>(out, ps, k, offsets, nb, width, vec, st);
    case PSG_F64: return launch_pool_reduce_mean<PSG_F64>(out, ps, k, offsets, nb, width, vec, st);
    case PSG_F16: return launch_pool_reduce_mean<PSG_F16>(out, ps, k, offsets, nb, width, vec, st);
    default: return launch_pool_reduce_mean<PSG_BF16>(out, ps, k, offsets, nb, width, vec, st);
  }
}

int psg_pool_scale_mean(float* dst, const float* grads, const uint64_t* offsets, uint64_t nb, uint32_t width,
                        psg_stream stream) {
  PSG_REQUIRE(width >= 1 && width <= 4096, PSG_ERR_INVALID, "psg_pool_scale_mean: width %u outside [1, 4096]", width);
  const uintptr_t d = reinterpret_cast<uintptr_t>(dst), g = reinterpret_cast<uintptr_t>(grads);
  if (nb) {
    PSG_REQUIRE(dst && grads, PSG_ERR_INVALID, "psg_pool_scale_mean: null dst or grads");
    PSG_REQUIRE(offsets, PSG_ERR_INVALID, "psg_pool_scale_mean: null offsets");
    PSG_REQUIRE((d | g) % 4 == 0, PSG_ERR_INVALID, "psg_pool_scale_mean: a pointer is not aligned to its 4-byte elements");
    PSG_REQUIRE(reinterpret_cast<uintptr_t>(offsets) % 8 == 0, PSG_ERR_INVALID,
                "psg_pool_scale_mean: offsets are not aligned to 8 bytes");
    PSG_REQUIRE(apart(d, g, (unsigned __int128)nb * width * 4), PSG_ERR_INVALID, "psg_pool_scale_mean: dst overlaps grads");
  }
  PSG_REQUIRE(nb <= kMaxRouted, PSG_ERR_RANGE, "psg_pool_scale_mean: %llu bags, more than 2^32-2", (unsigned long long)nb);
  if (nb == 0) return PSG_OK;
  const bool vec = width % 4 == 0 && (d | g) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  const BagGrid gr(nb, vec ? width / 4 : width);
  if (vec)
    k_pool_scale_mean<true><<<gr.blocks, kBlock, 0, st>>>((u32x4*)dst, (const u32x4*)grads, offsets, gr.units, gr.upr,
                                                          gr.dr, gr.dc);
  else
    k_pool_scale_mean<false><<<gr.blocks, kBlock, 0, st>>>(dst, grads, offsets, gr.units, gr.upr, gr.dr, gr.dc);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

}  // extern "C"
