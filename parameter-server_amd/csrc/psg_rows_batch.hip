// psg_rows_batch.hip — psg_table_lookup_pooled_batch: the pooled lookups of many
// row tables (psg_rows.hip) in one call.
//
// A model has tens to hundreds of embedding tables and needs a pooled bag from
// each of them every step.  One psg_table_lookup_pooled[_weighted] call a table
// is three launches, a clear, a copy and a host synchronisation whatever it
// moves; here the device work is fixed whatever the number of entries T:
//
//   descriptors H2D   one copy: two prefix arrays of T + 1 tile counts and T
//                     BatchEntry, built in a pinned mirror
//   gate clear        T x kRowFlags words, every entry its own
//   k_batch_front     every entry's offsets check AND any-order resolve
//   k_batch_pool<DT>  every entry's pooling, behind the entry's gate words
//   flags D2H, ONE host synchronisation
//
// Both kernels walk a FLATTENED TILE SPACE: the tiles of all entries laid end
// to end, prefix[i] the tiles in front of entry i.  A block strides over tiles,
// finds a tile's entry by a search of the prefix array (staged in LDS once a
// block; a block's tiles ascend, so the search starts at its last entry), and
// loads that entry's descriptor: block-uniform, so the index goes through
// readfirstlane and the descriptor lives in scalar registers.  The tile body
// is then the per-table kernel's, against that entry's arrays:
//
//   front  entry i's tiles are its offsets-check tiles (256 words each:
//          k_offsets_check's three rules) followed by its resolve tiles (kRowTile
//          keys each: k_rows_resolve_any's min/max bracket and side-by-side lower
//          bounds).  The two read nothing of each other's, so they share a
//          launch; slots go to the entry's base in the batch's slots array,
//          flags to gate[i * kRowFlags + ...].
//   pool   entry i's tiles are its (bag, unit) tiles, rows_per_tile(upr) bags
//          each, as k_rows_pool's.  A tile whose entry has a gate word raised is
//          skipped before one offset is read (the block goes on to its next
//          tile: it serves other entries too).  Else k_rows_pool's walk: slot
//          two ahead, row unit one ahead, the add; unit kind, pooling mode and
//          initializer are block-uniform branches from the descriptor.  One
//          writer per unit of the reply, no atomics.
//
// The tables are only read: keys, rows and the host fields of table_view.  The
// scratch (descriptors, slots, gate words, pinned mirrors) is the batch's own,
// per thread and GPU as psg_slice's, so a table may appear in any number of
// entries and no table's request scratch moves.
#include <algorithm>
#include <cstring>
#include <map>

#include "psg_internal.h"

namespace psg {
namespace {

constexpr uint64_t kMaxRows = 0xfffffffeull;
enum { kPoolSum = 0, kPoolWeighted = 1, kPoolMean = 2 };

// One request as the kernels read it (128 B, block-uniform).
struct BatchEntry {
  const uint64_t* keys;     // the request: n ids, nb + 1 offsets, n weights or null, the reply
  const uint64_t* offsets;
  const float* weights;
  void* out;
  const uint64_t* K;        // the table: S sorted keys, its rows, its key range
  const void* R;
  uint64_t S, kb, ke;
  uint64_t slot0;           // the entry's first word in the batch's slots array
  uint32_t n, nb;
  uint32_t upr, rpt;        // units a row, bags a pooling tile
  uint32_t vec, pool, init, pad;  // 16-B units; kPool*; absent ids add their initial rows
  InitSpec spec;
};
static_assert(sizeof(BatchEntry) == 128, "the descriptor is 128 B");

inline uint64_t check_tiles(uint64_t nb) { return nb ? (nb + kBlock) / kBlock : 0; }  // nb + 1 words, 256 a tile

// The prefix array into LDS; every lane returns with it staged.
__device__ __forceinline__ void stage_prefix(uint64_t* pre, const uint64_t* __restrict__ prefix, int T) {
  for (int j = threadIdx.x; j <= T; j += kBlock) pre[j] = prefix[j];
  __syncthreads();
}

// The entry of tile t: pre[i] <= t < pre[i + 1], searched from `from` (an entry
// at or in front of it) on; t < pre[T].  Every lane reads the same words of LDS.
__device__ __forceinline__ int entry_of(const uint64_t* pre, int from, int T, uint64_t t) {
  int lo = from, hi = T;  // pre[lo] <= t < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= t) lo = mid;
    else hi = mid;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ void raise(int* flags, int which, bool cond) {
  if (__ballot(cond) && (threadIdx.x & 63) == 0) flags[which] = 1;
}

// ---- kernel A: every entry's offsets check and resolve -----------------------------
__global__ __launch_bounds__(256) void k_batch_front(const BatchEntry* __restrict__ E,
                                                     const uint64_t* __restrict__ prefix, int T,
                                                     uint32_t* __restrict__ slots, int* __restrict__ gate) {
  constexpr int PER = kRowTile / kBlock;
  __shared__ uint64_t pre[PSG_BATCH_MAX + 1];
  __shared__ uint64_t wmin[kBlock / 64], wmax[kBlock / 64], win[2];
  stage_prefix(pre, prefix, T);
  const uint64_t total = pre[T];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int i = 0;
  for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
    i = entry_of(pre, i, T, t);
    const uint64_t lt = t - pre[i];
    const uint64_t n = E[i].n, nb = E[i].nb;
    int* flags = gate + (size_t)i * kRowFlags;
    const uint64_t nchk = (nb + kBlock) / kBlock;  // an entry with tiles has nb > 0
    if (lt < nchk) {
      // the three rules on 256 of the nb + 1 words: offsets[0] == 0, no offset
      // above its successor, offsets[nb] == n
      const uint64_t* __restrict__ offsets = E[i].offsets;
      const uint64_t b = lt * kBlock + threadIdx.x;
      bool bad = false;
      if (b <= nb) {
        const uint64_t o = offsets[b];
        bad = b == 0 && o != 0;
        if (b == nb ? o != n : offsets[b + 1] < o) bad = true;
      }
      raise(flags, kRowFlagOffsets, bad);
      continue;
    }
    // one tile of the any-order resolve against this entry's table
    const uint64_t* __restrict__ q = E[i].keys;
    const uint64_t* __restrict__ K = E[i].K;
    const uint64_t S = E[i].S, kb = E[i].kb, ke = E[i].ke;
    uint32_t* __restrict__ sl = slots + E[i].slot0;
    const uint64_t t0 = (lt - nchk) * kRowTile;
    const uint64_t t1 = t0 + kRowTile < n ? t0 + kRowTile : n;
    uint64_t key[PER];
    uint64_t mn = ~0ull, mx = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t j = t0 + (uint64_t)k * kBlock + threadIdx.x;
      key[k] = j < t1 ? q[j] : 0;
      if (j < t1) {
        mn = key[k] < mn ? key[k] : mn;
        mx = key[k] > mx ? key[k] : mx;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if (lane == 0) wmin[w] = mn, wmax[w] = mx;
    __syncthreads();
    if (w < 2) {  // wave 0 brackets the tile's minimum, wave 1 its maximum
      uint64_t x = w == 0 ? wmin[0] : wmax[0];
#pragma unroll
      for (int j = 1; j < kBlock / 64; ++j) {
        if (w == 0) x = wmin[j] < x ? wmin[j] : x;
        else x = wmax[j] > x ? wmax[j] : x;
      }
      uint64_t p = lower_bound_wave(K, S, x);
      if (w == 1) p = p < S ? p + 1 : S;
      if (lane == 0) win[w] = p;
    }
    __syncthreads();
    const uint64_t lo = win[0];
    const uint64_t hi = win[1] > lo ? win[1] : lo;
    // the lane's PER lower bounds in K[lo, hi) side by side: a step issues the PER
    // probes before it uses one; a probe K[base + half] has base + half < hi <= S
    uint64_t base[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) base[k] = lo;
    uint64_t len = hi - lo;
    while (len > 1) {
      const uint64_t half = len >> 1;
      uint64_t probe[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) probe[k] = K[base[k] + half];
#pragma unroll
      for (int k = 0; k < PER; ++k) base[k] = probe[k] < key[k] ? base[k] + half : base[k];
      len -= half;
    }
    bool range = false;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t j = t0 + (uint64_t)k * kBlock + threadIdx.x;
      if (j >= t1) continue;
      if (key[k] < kb || key[k] >= ke) range = true;
      bool found = false;
      uint64_t p = base[k];
      if (len == 1) {  // lower_bound is p, or p + 1 where K[p] < key
        const uint64_t x = K[p];
        found = x == key[k];
        if (x < key[k] && p + 1 < S) found = K[p + 1] == key[k], p = p + 1;
      }
      sl[j] = found ? (uint32_t)p : kRowAbsent;
    }
    raise(flags, kRowFlagRange, range);
    __syncthreads();  // wmin, wmax and win are the next tile's
  }
}

// ---- kernel B: every entry's pooling ---------------------------------------------------
// Pooling tile lt of one entry: k_rows_pool's walk over its rpt bags.  A lane
// takes (bag, unit) pairs, walks its bag's slots in arrival order and stores
// once.  `init`: an absent slot's unit is made from its key (InitUnit) and added
// like a row; else it loads nothing and adds nothing.
template <int DT, bool VEC, int POOL>
__device__ __forceinline__ void pool_tile(const BatchEntry* __restrict__ e, const uint32_t* __restrict__ slots,
                                          uint64_t lt) {
  using ACC = PoolAcc<DT, VEC>;
  using U = typename ACC::U;
  using INIT = InitUnit<DT, VEC>;
  static_assert(sizeof(U) == sizeof(typename INIT::U), "one unit size");
  const U* __restrict__ R = (const U*)e->R;
  U* __restrict__ out = (U*)e->out;
  const uint64_t* __restrict__ q = e->keys;
  const uint64_t* __restrict__ offsets = e->offsets;
  [[maybe_unused]] const float* __restrict__ weights = e->weights;
  const uint32_t* __restrict__ sl = slots + e->slot0;
  const uint32_t upr = e->upr, rpt = e->rpt;
  const bool init = e->init != 0;
  const InitSpec spec = e->spec;
  const uint64_t nb = e->nb;
  const uint64_t b0 = lt * rpt;
  const uint32_t nr = (uint32_t)(nb - b0 < rpt ? nb - b0 : rpt);
  const uint32_t total = nr * upr;
  RowWalk w(threadIdx.x, upr);
  for (uint32_t x = threadIdx.x; x < total; x += kBlock, w.next()) {
    const uint64_t b = b0 + w.r;
    const uint32_t c = w.c;
    uint32_t p = (uint32_t)offsets[b];  // <= n <= 2^32 - 2: checked by the front
    const uint32_t pe = (uint32_t)offsets[b + 1];
    [[maybe_unused]] const uint32_t len = pe - p;
    auto unit_at = [&](uint32_t slot, uint32_t pos) -> U {
      if (slot != kRowAbsent) return R[(uint64_t)slot * upr + c];
      if (init) return __builtin_bit_cast(U, INIT::make(q[pos], c, spec));
      return U{};
    };
    typename ACC::A acc = {};  // +0
    if (p < pe) {
      uint32_t s0 = sl[p];
      uint32_t s1 = p + 1 < pe ? sl[p + 1] : kRowAbsent;
      [[maybe_unused]] float w0 = 0, w1 = 0;
      if constexpr (POOL == kPoolWeighted) {
        w0 = weights[p];
        if (p + 1 < pe) w1 = weights[p + 1];
      }
      U v = unit_at(s0, p);
      for (; p < pe; ++p) {
        const uint32_t s2 = p + 2 < pe ? sl[p + 2] : kRowAbsent;
        [[maybe_unused]] float w2 = 0;
        if constexpr (POOL == kPoolWeighted)
          if (p + 2 < pe) w2 = weights[p + 2];
        U vn = {};
        if (p + 1 < pe) vn = unit_at(s1, p + 1);
        if (init || s0 != kRowAbsent) {
          if constexpr (POOL == kPoolWeighted) acc = ACC::sum(acc, ACC::times(w0, v));
          else acc = ACC::add(acc, v);
        }
        if constexpr (POOL == kPoolWeighted) w0 = w1, w1 = w2;
        s0 = s1, s1 = s2, v = vn;
      }
      if constexpr (POOL == kPoolMean) acc = ACC::over(acc, len);
    }
    out[b * upr + c] = ACC::round(acc);
  }
}

template <int DT, bool VEC>
__device__ __forceinline__ void pool_tile_mode(const BatchEntry* __restrict__ e, const uint32_t* __restrict__ slots,
                                               uint64_t lt) {
  const uint32_t pool = e->pool;
  if (pool == kPoolWeighted) pool_tile<DT, VEC, kPoolWeighted>(e, slots, lt);
  else if (pool == kPoolMean) pool_tile<DT, VEC, kPoolMean>(e, slots, lt);
  else pool_tile<DT, VEC, kPoolSum>(e, slots, lt);
}

template <int DT>
__global__ __launch_bounds__(256) void k_batch_pool(const BatchEntry* __restrict__ E,
                                                    const uint64_t* __restrict__ prefix, int T,
                                                    const uint32_t* __restrict__ slots,
                                                    const int* __restrict__ gate) {
  __shared__ uint64_t pre[PSG_BATCH_MAX + 1];
  stage_prefix(pre, prefix, T);
  const uint64_t total = pre[T];
  int i = 0;
  for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
    i = entry_of(pre, i, T, t);
    const int* g = gate + (size_t)i * kRowFlags;
    if (g[kRowFlagRange] | g[kRowFlagOffsets]) continue;  // a refused entry: not one offset is read
    const uint64_t lt = t - pre[i];
    if (E[i].vec) pool_tile_mode<DT, true>(E + i, slots, lt);
    else pool_tile_mode<DT, false>(E + i, slots, lt);
  }
}

// ---- the host side ----------------------------------------------------------------------
// Per-thread, per-GPU scratch of the batch, kept for the thread's lifetime: the
// descriptor block and the gate words for PSG_BATCH_MAX entries with their pinned
// mirrors (allocated once), and the slots array (grown to the largest sum(ns)).
constexpr size_t kDescBytes = 2 * (PSG_BATCH_MAX + 1) * sizeof(uint64_t) + PSG_BATCH_MAX * sizeof(BatchEntry);
constexpr size_t kGateBytes = (size_t)PSG_BATCH_MAX * kRowFlags * sizeof(int);
struct BatchScratch {
  char* desc_dev = nullptr;
  char* desc_host = nullptr;
  int* gate = nullptr;
  int* flags_host = nullptr;
  uint32_t* slots = nullptr;
  uint64_t slots_cap = 0;
};
thread_local std::map<int, BatchScratch> t_batch_scratch;

int get_batch_scratch(uint64_t nslots, BatchScratch** out) {
  int dev = 0;
  PSG_HIP(hipGetDevice(&dev));
  BatchScratch& s = t_batch_scratch[dev];
  if (!s.desc_dev) PSG_HIP(hipMalloc((void**)&s.desc_dev, kDescBytes));
  if (!s.desc_host) PSG_HIP(hipHostMalloc((void**)&s.desc_host, kDescBytes, hipHostMallocDefault));
  if (!s.gate) PSG_HIP(hipMalloc((void**)&s.gate, kGateBytes));
  if (!s.flags_host) PSG_HIP(hipHostMalloc((void**)&s.flags_host, kGateBytes, hipHostMallocDefault));
  if (s.slots_cap < nslots) {
    if (s.slots) PSG_HIP(hipFree(s.slots));
    s.slots = nullptr;
    s.slots_cap = 0;
    const uint64_t cap = std::max<uint64_t>(nslots, 1 << 16);
    PSG_HIP(hipMalloc((void**)&s.slots, cap * sizeof(uint32_t)));
    s.slots_cap = cap;
  }
  *out = &s;
  return PSG_OK;
}

unsigned grid_for(uint64_t tiles) {
  const uint64_t cap = (uint64_t)max_stream_blocks();
  return (unsigned)(tiles < cap ? tiles : cap);
}

int launch_pool(int dtype, unsigned grid, const BatchEntry* E, const uint64_t* prefix, int T, const uint32_t* slots,
                const int* gate, hipStream_t st) {
  switch (dtype) {
    case PSG_F32: k_batch_pool<PSG_F32><<<grid, kBlock, 0, st>>>(E, prefix, T, slots, gate); break;
    case PSG_F64: k_batch_pool<PSG_F64><<<grid, kBlock, 0, st>>>(E, prefix, T, slots, gate); break;
    case PSG_F16: k_batch_pool<PSG_F16><<<grid, kBlock, 0, st>>>(E, prefix, T, slots, gate); break;
    default: k_batch_pool<PSG_BF16><<<grid, kBlock, 0, st>>>(E, prefix, T, slots, gate); break;
  }
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

}  // namespace
}  // namespace psg

using namespace psg;

extern "C" int psg_table_lookup_pooled_batch(int T, psg_table* const* tables_host, const uint64_t* const* keys_host,
                                             const uint64_t* const* offsets_host, const float* const* weights_host,
                                             const int* modes_host, void* const* outs_host, const uint64_t* ns_host,
                                             const uint64_t* nbs_host, psg_stream stream, int* status_host) {
  const char* name = "psg_table_lookup_pooled_batch";
  PSG_REQUIRE(T >= 1 && T <= PSG_BATCH_MAX, PSG_ERR_INVALID, "%s: %d entries outside [1, %d]", name, T, PSG_BATCH_MAX);
  PSG_REQUIRE(tables_host, PSG_ERR_INVALID, "%s: null tables array", name);
  PSG_REQUIRE(keys_host, PSG_ERR_INVALID, "%s: null keys array", name);
  PSG_REQUIRE(offsets_host, PSG_ERR_INVALID, "%s: null offsets array", name);
  PSG_REQUIRE(modes_host, PSG_ERR_INVALID, "%s: null modes array", name);
  PSG_REQUIRE(outs_host, PSG_ERR_INVALID, "%s: null outs array", name);
  PSG_REQUIRE(ns_host, PSG_ERR_INVALID, "%s: null ns array", name);
  PSG_REQUIRE(nbs_host, PSG_ERR_INVALID, "%s: null nbs array", name);
  for (int i = 0; i < T; ++i) {
    const uint64_t n = ns_host[i], nb = nbs_host[i];
    const float* weights = weights_host ? weights_host[i] : nullptr;
    const int mode = modes_host[i];
    PSG_REQUIRE(tables_host[i], PSG_ERR_INVALID, "%s: null table of entry %d", name, i);
    PSG_REQUIRE(keys_host[i] || n == 0, PSG_ERR_INVALID, "%s: null keys of entry %d", name, i);
    PSG_REQUIRE(offsets_host[i] || nb == 0, PSG_ERR_INVALID, "%s: null offsets of entry %d", name, i);
    PSG_REQUIRE(outs_host[i] || nb == 0, PSG_ERR_INVALID, "%s: null out of entry %d", name, i);
    PSG_REQUIRE(nb > 0 || n == 0, PSG_ERR_INVALID, "%s: %llu keys and no bag to hold them in entry %d", name,
                (unsigned long long)n, i);
    PSG_REQUIRE(mode == PSG_POOL_SUM || mode == PSG_POOL_MEAN, PSG_ERR_INVALID,
                "%s: mode %d of entry %d is no pooling mode", name, mode, i);
    PSG_REQUIRE(mode != PSG_POOL_MEAN || !weights, PSG_ERR_INVALID, "%s: weights with PSG_POOL_MEAN in entry %d", name,
                i);
    PSG_REQUIRE((reinterpret_cast<uintptr_t>(weights) & 3u) == 0, PSG_ERR_INVALID,
                "%s: weights of entry %d not on a 4-B boundary", name, i);
  }
  for (int i = 0; i < T; ++i)
    PSG_REQUIRE(ns_host[i] <= kMaxRows && nbs_host[i] <= kMaxRows, PSG_ERR_RANGE,
                "%s: more than 2^32-2 keys or bags in entry %d", name, i);
  const int dtype = table_view(tables_host[0]).dtype;
  for (int i = 1; i < T; ++i)
    PSG_REQUIRE(table_view(tables_host[i]).dtype == dtype, PSG_ERR_UNSUPPORTED,
                "%s: entry %d's table has dtype %d, entry 0's has %d (one dtype a call)", name, i,
                table_view(tables_host[i]).dtype, dtype);

  uint64_t nslots = 0, served = 0;
  for (int i = 0; i < T; ++i) nslots += ns_host[i], served += nbs_host[i];
  if (served == 0) {  // every entry a no-op
    if (status_host) std::fill(status_host, status_host + T, (int)PSG_OK);
    return PSG_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  BatchScratch* sc = nullptr;
  PSG_TRY(get_batch_scratch(nslots, &sc));

  // the descriptor block: front prefix, pool prefix, entries
  const size_t entries_at = 2 * (size_t)(T + 1) * sizeof(uint64_t);
  const size_t bytes = entries_at + (size_t)T * sizeof(BatchEntry);
  uint64_t* pre_front = (uint64_t*)sc->desc_host;
  uint64_t* pre_pool = pre_front + (T + 1);
  BatchEntry* E = (BatchEntry*)(sc->desc_host + entries_at);
  const int esize = dtype_size(dtype);
  uint64_t slot0 = 0, tf = 0, tp = 0;
  for (int i = 0; i < T; ++i) {
    const TableView v = table_view(tables_host[i]);
    const uint64_t n = ns_host[i], nb = nbs_host[i];
    const float* weights = weights_host ? weights_host[i] : nullptr;
    // 16-B units under accumulate_vec's condition for a Pull
    const bool vec = ((uint64_t)v.width * esize) % 16 == 0 && aligned16(outs_host[i]);
    BatchEntry& e = E[i];
    e.keys = keys_host[i], e.offsets = offsets_host[i], e.weights = weights, e.out = outs_host[i];
    e.K = v.keys, e.R = v.rows, e.S = v.size, e.kb = v.key_begin, e.ke = v.key_end;
    e.slot0 = slot0;
    e.n = (uint32_t)n, e.nb = (uint32_t)nb;
    e.upr = vec ? v.width * (uint32_t)esize / 16 : v.width;
    e.rpt = rows_per_tile(e.upr);
    e.vec = vec, e.pad = 0;
    e.pool = modes_host[i] == PSG_POOL_MEAN ? kPoolMean : weights ? kPoolWeighted : kPoolSum;
    e.init = v.init_kind == PSG_INIT_UNIFORM;
    e.spec = init_spec(v.init_seed, v.init_lo, v.init_hi);
    pre_front[i] = tf, pre_pool[i] = tp;
    if (nb) {
      tf += check_tiles(nb) + (n + kRowTile - 1) / kRowTile;
      tp += (nb + e.rpt - 1) / e.rpt;
    }
    slot0 += n;
  }
  pre_front[T] = tf, pre_pool[T] = tp;

  const uint64_t* d_front = (const uint64_t*)sc->desc_dev;
  const uint64_t* d_pool = d_front + (T + 1);
  const BatchEntry* d_E = (const BatchEntry*)(sc->desc_dev + entries_at);
  const size_t gate_bytes = (size_t)T * kRowFlags * sizeof(int);
  PSG_HIP(hipMemcpyAsync(sc->desc_dev, sc->desc_host, bytes, hipMemcpyHostToDevice, st));
  PSG_HIP(hipMemsetAsync(sc->gate, 0, gate_bytes, st));
  k_batch_front<<<grid_for(tf), kBlock, 0, st>>>(d_E, d_front, T, sc->slots, sc->gate);
  PSG_HIP(hipGetLastError());
  PSG_TRY(launch_pool(dtype, grid_for(tp), d_E, d_pool, T, sc->slots, sc->gate, st));
  // the one synchronisation: the requests no longer read, the replies in memory, the flags on the host
  PSG_HIP(hipMemcpyAsync(sc->flags_host, sc->gate, gate_bytes, hipMemcpyDeviceToHost, st));
  PSG_HIP(hipStreamSynchronize(st));

  int rc = PSG_OK;
  for (int i = 0; i < T; ++i) {
    const int* f = sc->flags_host + (size_t)i * kRowFlags;
    const int s = f[kRowFlagOffsets] ? PSG_ERR_INVALID : f[kRowFlagRange] ? PSG_ERR_RANGE : PSG_OK;
    if (status_host) status_host[i] = s;
    if (s == PSG_OK || rc != PSG_OK) continue;
    rc = s;
    if (s == PSG_ERR_INVALID)
      set_error("%s: offsets of entry %d do not start at 0, ascend and end at n = %llu", name, i,
                (unsigned long long)ns_host[i]);
    else
      set_error("%s: a key of entry %d lies outside its table's range", name, i);
  }
  return rc;
}
