// psg_store.hip — the server-side value store in HBM and the request handle.
//
// Replaces `std::unordered_map<Key, Value> store` of KVServerDefaultHandle
// (src/ps/KVApp.h:433-458).  Two layouts:
//
//   DENSE   one value array; key k at slot k - key_begin.  A request with
//           consecutive keys (keys == NULL) is one streaming kernel
//           (psg_dense.hip).
//   SORTED  a sorted uint64 key array K[0..size) and a value array V in the
//           same order.  A request (sorted, unique keys — the KVPairs contract,
//           KVApp.h:23) runs as two kernels:
//             k_validate_windows  reads every request key once (coalesced):
//               strictly ascending and inside the shard's range, or the whole
//               request is rejected before anything is written; and, per
//               request tile, the window of K its first and last key bracket
//               (one 64-ary search per tile end) — skipped when the windows
//               cached for this key array are trusted (below);
//             k_resolve_apply     stages each tile's window of K into LDS,
//               places every key by an LDS search / merge walk and applies the
//               request to the found slots (store[slot] += val, out = store),
//               then signals the request's completion itself (block_arrive).
//           A tile's window depends only on K and the tile's first and last
//           key, so windows are cached per request key array (the LR and
//           benchmark steady state repeats one key list): k_resolve_apply
//           checks each cached window against its tile's end keys and, on a
//           mismatch, searches it inline.  A Pull on trusted windows is ONE
//           kernel; a Push is the key-stream validation plus that kernel.
//           Keys that are absent are inserted with value 0 afterwards — the
//           `operator[]` insert of KVApp.h:449/452 — by a parallel merge of the
//           (compacted, sorted) new keys into K and V, and the request is
//           applied to exactly those keys.
//   Rejected requests (unsorted, duplicate, out-of-range keys) leave the store
//   unchanged: the validation pass raises a device word that every
//   store-writing kernel of the request checks first.  A Pull, which writes
//   only its reply, skips that pass: k_resolve_apply checks its keys on the
//   way (the reply of a rejected Pull is unspecified, as no reply is sent).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "psg_internal.h"

namespace psg {

constexpr int kTile = 1024;  // request keys per block tile (4 per lane)

constexpr uint32_t kNoSlot = 0xffffffffu;

// Request flags of the launches that report through the stream (the
// two-pass resolve, the DENSE-keyed check, psg_store_resolve): pinned host ints
// the kernels set (one store of 1 per wave that saw the condition —
// idempotent, no atomics), zeroed by the host before the launch and read once
// an event recorded behind the launch has completed (read_flags = stream_done:
// the completed event promises what a stream synchronisation promises).
// F_WINMISS: a cached window did not match its tile (searched inline).
enum { F_MISSING = 0, F_WINMISS = 1, F_RANGE = 2, F_UNSORTED = 3, F_NFLAGS = 4 };

__device__ __forceinline__ void raise_flag(int* flags, int which, bool cond) {
  if (__ballot(cond) && (threadIdx.x & 63) == 0) flags[which] = 1;
}

// The fused keyed request (k_resolve_apply) reports through ONE word of the
// store's ring in pinned host memory: bits [8, 32) the request's 24-bit tag,
// bits [0, 8) its flags:
enum {
  W_MISSING = 1,
  W_WINMISS = 2,
  W_RANGE = 4,
  W_UNSORTED = 8,
  W_GATED = 16,
  W_NOTIDENT = 32,
  W_PARTIAL = 64,
  W_NOTLIST = 128
};
// Device words (reject_dev): the validation pass writes a request's sequence
// number into [kRejRange] / [kRejUnsorted] when a key is out of the shard's
// range / out of order.  [kPending] != 0: an earlier request needs the host
// first (absent keys to insert, or keys out of order to take the
// order-preserving path); every later fused request then writes nothing and
// reports W_GATED, and the host replays it after that follow-up.
// [kRejIdent]: an identity request's check (k_ident_check) failed.
constexpr int kRejRange = 0, kRejUnsorted = 1, kPending = 2, kRejIdent = 3;
// [kFramesBase, +2): a uint64 — the stretch base of a run of Pushes
// (psg_store_push_frames, frames_base), read by its check and apply kernels.
constexpr int kFramesBase = 8;
// [kRejRun]: a strided run's check pass found a key off its slot (psg_runs.hip)
constexpr int kRejRun = 4;
// [kRejList]: a Push sent as its list's verified copy was not that list
// (k_list_check; the lean apply then writes nothing and reports W_NOTLIST)
constexpr int kRejList = 5;

// The store-key window of one request tile: [lo, hi) of K brackets every key
// between the tile's first and last key (lo = lower_bound(K, first), hi =
// lower_bound(K, last) + 1, clipped to S).  Valid while K is unchanged (gen).
struct Win {
  uint64_t first, last;
  uint32_t lo, hi, gen, pad;
};

// Tile words and lane codes (round 5, coded tiles).  tword[t] = (seq & 2^30-1)
// << 2 | st for the request `seq`: st 2 = the tile is a stretch of the store
// (key i at slot lo + i), 1 = a coded tile (every key found; lane l's code in
// codes[t * 1024 + l]), 0 = the general path.  A word of another request means
// a stretch (k_validate_windows marks only the tiles that are not).
constexpr uint32_t kTileGeneral = 0, kTileCoded = 1, kTileStretch = 2, kTileDone = 3;
__device__ __forceinline__ uint32_t tile_tag(int seq) { return ((uint32_t)seq & 0x3fffffffu) << 2; }

// Completion of a fused request and its flags, ordered by atomicity alone.
// Every block adds ONE 64-bit value to one of 8 shard counters (blockIdx mod
// 8, each on its own 256 B, so 2048 arrivals do not queue on one address): 1
// in bits [0, 12), plus 1 in the field of each condition it saw — absent keys
// [12, 24), a stale window [24, 36), and for a Pull, which checks its own
// keys, a key out of range [36, 48) or out of order [48, 60).  The block whose
// add completes its shard (the value the add returned says so) adds its
// shard's conditions, as one more such value, to the top counter; the block
// that completes the top writes the completion word — tag and flags in ONE
// system-scope store — and zeroes the counters (every block of the launch has
// arrived: no add can follow).  Each request of the ring has its own counter
// set, used again kRing requests later.  A read-modify-write
// returns the latest value of its counter, so the completing sum holds every
// block's conditions and the word is right by atomicity: no fence, and the
// host reads nothing but that word.  The apply stores need no ordering here:
// only later launches on the same stream read them.  (A posted per-block word
// in host memory instead — no atomic — took 50-90 us to land for 2048 blocks:
// PCIe writes serialise.)
constexpr int kArriveShards = 8;
constexpr int kArriveStride = 32;  // 64-bit words between counters (256 B)
constexpr int kField = 12;
constexpr uint64_t kFieldMask = (1ull << kField) - 1;
struct Arrival {
  uint64_t* ctr;  // kArriveShards shard counters, then the top counter
};
// blocks of the launch that arrive on shard j, and shards that receive any
__device__ __forceinline__ uint32_t shard_blocks(uint32_t j) {
  return gridDim.x > j ? (gridDim.x - 1 - j) / kArriveShards + 1 : 0;
}
__device__ __forceinline__ uint32_t used_shards() {
  return gridDim.x < (uint32_t)kArriveShards ? gridDim.x : (uint32_t)kArriveShards;
}
// cond bits: 1 absent key, 2 stale window, 4 out of range, 8 out of order
__device__ __forceinline__ uint64_t arrival_value(uint32_t cond) {
  uint64_t a = 1;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (cond & (1u << k)) a += 1ull << ((k + 1) * kField);
  return a;
}
__device__ __forceinline__ uint32_t sum_conditions(uint64_t sum) {
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((sum >> ((k + 1) * kField)) & kFieldMask) c |= 1u << k;
  return c;
}
// Block arrival once every condition of the block is known (after the resolve
// of its last tile): the block's threads OR theirs into an LDS word (zeroed at
// kernel start, before a barrier), and thread 0 adds the block's value to its
// shard.  Returns the shard's count after this add (thread 0).
__device__ __forceinline__ uint64_t block_arrive(uint32_t cond, uint32_t* s_cond, const Arrival& a) {
  if (cond) atomicOr(s_cond, cond);
  __syncthreads();
  uint64_t after = 0;
  if (threadIdx.x == 0) {
    const uint64_t v = arrival_value(*s_cond);
    after = __hip_atomic_fetch_add(a.ctr + (blockIdx.x % kArriveShards) * kArriveStride, v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT) + v;
  }
  return after;
}
// uniform: flags every block knows alike (W_GATED, and a Push's rejection
// read from the reject words); kPending is raised when the request needs the
// host's follow-up (absent keys, keys out of order, or an identity request
// that was not one, and not rejected).  c2: the flag condition bit 2 reports
// (W_WINMISS; W_NOTIDENT for the identity kernel).
__device__ __forceinline__ void request_done(uint64_t after, const Arrival& a, uint32_t uniform, int* pending,
                                             uint32_t* word, uint32_t tag_bits, uint32_t c2 = W_WINMISS) {
  if (threadIdx.x != 0 || (after & kFieldMask) != shard_blocks(blockIdx.x % kArriveShards)) return;
  const uint64_t v = arrival_value(sum_conditions(after));  // the shard's conditions, counted once
  const uint64_t top =
      __hip_atomic_fetch_add(a.ctr + kArriveShards * kArriveStride, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + v;
  if ((top & kFieldMask) != used_shards()) return;
  const uint32_t c = sum_conditions(top);
  uint32_t f = uniform;
  if (c & 1u) f |= W_MISSING;
  if (c & 2u) f |= c2;
  if (c & 4u) f |= W_RANGE;
  if (c & 8u) f |= W_UNSORTED;
  // zeroed by read-modify-writes, like the adds (one point of coherence for
  // all of a counter's accesses); the set is next used kRing requests later
  for (int k = 0; k <= kArriveShards; ++k)
    (void)__hip_atomic_exchange(a.ctr + k * kArriveStride, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!(f & (W_GATED | W_RANGE)) && (f & (W_MISSING | W_UNSORTED | W_NOTIDENT | W_PARTIAL | W_NOTLIST)))
    __hip_atomic_store(pending, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(word, tag_bits | f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// lower_bound_dev: psg_internal.h

// spare elements after a store's keys: k_resolve_apply's 16-B LDS loads may
// read 8 B past the last key
constexpr uint64_t kKeyPad = 2;
constexpr int kWin = 2048;  // LDS-staged window of store keys (16 KiB: 10 blocks per CU)

// lower_bound_wave: psg_internal.h

// Pass 1: the store-key window of every 1024-key request tile, one wave per
// tile: wlo[t] = lower_bound(K, q[t * kTile]); wlo[ntiles] = lower_bound(K, q[n-1]) + 1.
__global__ __launch_bounds__(256) void k_tile_windows(const uint64_t* __restrict__ q, uint64_t n,
                                                      const uint64_t* __restrict__ K, uint64_t S,
                                                      uint64_t* __restrict__ wlo, uint64_t tile) {
  const uint64_t ntiles = (n + tile - 1) / tile;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
  for (uint64_t t = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t <= ntiles; t += waves) {
    if (t < ntiles) {
      const uint64_t r = lower_bound_wave(K, S, q[t * tile]);
      if ((threadIdx.x & 63) == 0) wlo[t] = r;
    } else {
      const uint64_t h = lower_bound_wave(K, S, q[n - 1]);
      if ((threadIdx.x & 63) == 0) wlo[t] = h < S ? h + 1 : S;
    }
  }
}

__device__ __forceinline__ uint32_t lower_bound_lds(const uint64_t* a, uint32_t w, uint64_t key) {
  uint32_t lo = 0, hi = w;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Pass 2: resolve sorted request keys q[0..n) against K[0..S).  Each block
// stages its tile's window of K into LDS with coalesced loads; every lane then
// owns 4 consecutive request keys: one LDS binary search places the first,
// and each next key (larger, since q is ascending) is placed by a merge walk —
// it is almost always at the previous position or the one after, two LDS
// reads — with a binary search of the rest of the window as the fallback.  A
// global search is used only when a sparse request leaves a window wider than
// kWin.  slots[i] = index of q[i] in K, or kNoSlot.  flags: [F_MISSING] |=
// absent keys, [F_RANGE] |= key outside [kb, ke), [F_UNSORTED] |= q not
// strictly ascending.  A slot is only
// written when K[slot] == key, so unsorted input never produces a wrong slot
// (it is flagged and the request rejected).
constexpr int kPerLane = kTile / kBlock;  // 4 consecutive keys per lane

__global__ __launch_bounds__(256) void k_resolve(const uint64_t* __restrict__ q, uint64_t n,
                                                 const uint64_t* __restrict__ K, uint64_t S,
                                                 const uint64_t* __restrict__ wlo, uint64_t kb,
                                                 uint64_t ke, uint32_t* __restrict__ slots,
                                                 int* __restrict__ flags) {
  __shared__ uint64_t sK[kWin];
  int missing = 0, range = 0, unsorted = 0;
  const uint64_t ntiles = (n + kTile - 1) / kTile;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * kTile;
    const uint64_t t1 = (t0 + kTile < n) ? t0 + kTile : n;
    const uint64_t lo = wlo[tile];
    uint64_t hi = tile + 1 < ntiles ? wlo[tile + 1] + 1 : wlo[ntiles];
    if (hi > S) hi = S;
    if (hi < lo) hi = lo;  // unsorted input
    const uint64_t W = hi - lo;
    const bool staged = W <= (uint64_t)kWin;
    if (staged)
      for (uint64_t j = threadIdx.x; j < W; j += kBlock) sK[j] = K[lo + j];
    __syncthreads();
    const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kPerLane;
    uint64_t prev = i0 > 0 && i0 < t1 ? q[i0 - 1] : 0;
    uint32_t r = 0;  // lower bound of the previous key inside the window
    uint32_t out[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const uint64_t i = i0 + k;
      out[k] = kNoSlot;
      if (i >= t1) continue;
      const uint64_t key = q[i];
      if (key < kb || key >= ke) range = 1;
      if (i > 0 && prev >= key) unsorted = 1;
      prev = key;
      uint64_t p;
      bool found;
      if (staged) {
        const uint32_t w = (uint32_t)W;
        if (k == 0) {
          r = lower_bound_lds(sK, w, key);
        } else if (!(r < w && sK[r] >= key)) {
          if (r + 1 < w && sK[r + 1] >= key) r = r + 1;  // the next store key
          else r = (r + 1 >= w) ? w : r + 1 + lower_bound_lds(sK + r + 1, w - r - 1, key);
        }
        p = lo + r;
        found = r < w && sK[r] == key;
      } else {
        p = lower_bound_dev(K, lo, hi, key);
        found = p < S && K[p] == key;
      }
      out[k] = found ? (uint32_t)p : kNoSlot;
      if (!found) missing++;
    }
    if (i0 + kPerLane <= t1 && ((i0 & 3) == 0)) {
      // 16-B store of the lane's 4 slots (slots is our own 256-B aligned buffer)
      *reinterpret_cast<u32x4*>(slots + i0) = u32x4{out[0], out[1], out[2], out[3]};
    } else {
      for (int k = 0; k < kPerLane; ++k)
        if (i0 + k < t1) slots[i0 + k] = out[k];
    }
    __syncthreads();
  }
  raise_flag(flags, F_MISSING, missing != 0);
  raise_flag(flags, F_RANGE, range != 0);
  raise_flag(flags, F_UNSORTED, unsorted != 0);
}

// Pass 1 of a SORTED request: validate the whole request and find each
// tile's window of K, as two kinds of 256-thread blocks of one launch:
//   blocks [0, nsearch)  one wave per window bound: win[t].lo = lower_bound(K,
//                        first key of tile t), win[t].hi = lower_bound(K, last
//                        key of tile t) + 1 (a 64-ary search each, ~4
//                        dependent scattered probes of 512 B), tagged with K's
//                        generation and the two keys;
//   the other blocks     stream the request keys (8 per lane, 16-B loads) and
//                        check strict ascent — against the key before each
//                        lane's eight — and the shard's range [kb, ke).
// Either kind may be absent (nsearch = 0: the windows cached for this key
// array are trusted; no stream blocks: a Pull, which checks its own keys).
// The search blocks come first in dispatch order, so their latency runs under
// the key stream.  An invalid request writes seq into reject[kRejRange] /
// [kRejUnsorted], which k_resolve_apply checks before it writes anything and
// reports in the request's completion word.  Bytes: the request keys once (8 B / key, default
// cache policy so k_resolve_apply's re-read right after can hit the Infinity
// Cache) plus the probes.
//
// Tiles that are stretches of the store (round 5).  With trusted windows and
// chunk_ok != NULL, the key-stream blocks also check, per 512-key wave chunk,
// whether its tile's keys are exactly K[lo, lo + n_t) — the tile's window holds
// exactly n_t store keys, its end keys are the window's, and every key equals
// its store key — reading those store keys (8 B / key) beside the request keys
// they already read.  A chunk that is not writes seq into its tile's word
// chunk_ok[t]; k_resolve_apply then serves a tile whose word is not seq at
// slots lo + i, with no key
// re-read, no window and no search: a key list made of stretches of the store
// (a few disjoint ranges of it) moves 8 + 8 + 4 + 8 = 28 B per key in its
// stretch tiles, where the general path moves 36 — only the tiles that hold a
// seam between two stretches take the general path.
__global__ __launch_bounds__(256) void k_validate_windows(const uint64_t* __restrict__ q, uint64_t n,
                                                          const uint64_t* __restrict__ K, uint64_t S,
                                                          Win* __restrict__ win, uint32_t gen, uint64_t tileN,
                                                          unsigned nsearch, uint64_t kb, uint64_t ke,
                                                          int* __restrict__ reject, int seq, int vec,
                                                          int* __restrict__ chunk_ok) {
  const uint64_t ntiles = (n + tileN - 1) / tileN;
  if (blockIdx.x < nsearch) {
    const uint64_t waves = (uint64_t)nsearch * (kBlock / 64);
    for (uint64_t b = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); b < 2 * ntiles; b += waves) {
      const uint64_t t = b >> 1;
      const uint64_t t1 = (t + 1) * tileN < n ? (t + 1) * tileN : n;
      if ((b & 1) == 0) {
        const uint64_t key = q[t * tileN];
        const uint64_t r = lower_bound_wave(K, S, key);
        if ((threadIdx.x & 63) == 0) {
          win[t].first = key;
          win[t].lo = (uint32_t)r;
          win[t].gen = gen;
        }
      } else {
        const uint64_t key = q[t1 - 1];
        const uint64_t h = lower_bound_wave(K, S, key);
        if ((threadIdx.x & 63) == 0) {
          win[t].last = key;
          win[t].hi = (uint32_t)(h < S ? h + 1 : S);
        }
      }
    }
    return;
  }
  // Each wave checks 512 consecutive keys as 4 rows of 128: row h's load is
  // one contiguous KiB (lane l holds keys 2l, 2l+1 of the row, one 16-B
  // load), and the 4 loads are in flight together.  The key before a lane's
  // pair is the previous lane's second (a shuffle), the previous row's last
  // (lane 63's, broadcast) for lane 0, and for row 0 the key before the
  // wave's run, which lane 0 loads.  The loop bound is block-uniform (the
  // shuffles need every lane).
  constexpr int kRows = 4, kRowKeys = 128, kWaveKeys = kRows * kRowKeys;
  int range = 0, unsorted = 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t nvb = (uint64_t)gridDim.x - nsearch;
  constexpr uint64_t kBlockKeys = (uint64_t)(kBlock / 64) * kWaveKeys;  // 2048
  for (uint64_t base = (uint64_t)(blockIdx.x - nsearch) * kBlockKeys; base < n; base += nvb * kBlockKeys) {
    const uint64_t wbase = base + (uint64_t)wv * kWaveKeys;
    // the chunk's tile window, read first: its latency runs under the key loads
    Win e = {};
    if (chunk_ok && wbase < n) e = win[wbase / tileN];
    uint64_t k0[kRows], k1[kRows];
#pragma unroll
    for (int h = 0; h < kRows; ++h) {
      const uint64_t i = wbase + (uint64_t)h * kRowKeys + 2 * (uint64_t)lane;
      if (i + 2 <= n && vec) {
        const u64x2 a = *reinterpret_cast<const u64x2*>(q + i);
        k0[h] = a[0];
        k1[h] = a[1];
      } else {
        k0[h] = i < n ? q[i] : 0;
        k1[h] = i + 1 < n ? q[i + 1] : 0;
      }
    }
    uint64_t before = 0;  // the key before the wave's run (lane 0)
    if (lane == 0 && wbase > 0 && wbase < n) before = q[wbase - 1];
#pragma unroll
    for (int h = 0; h < kRows; ++h) {
      const uint64_t i = wbase + (uint64_t)h * kRowKeys + 2 * (uint64_t)lane;
      const uint32_t plo = __shfl_up((uint32_t)k1[h], 1, 64), phi = __shfl_up((uint32_t)(k1[h] >> 32), 1, 64);
      uint64_t prev = ((uint64_t)phi << 32) | plo;
      uint64_t row_before = before;  // (h is unrolled: every lane runs the broadcast)
      if (h > 0) {
        const uint32_t llo = __shfl((uint32_t)k1[h - 1], 63, 64), lhi = __shfl((uint32_t)(k1[h - 1] >> 32), 63, 64);
        row_before = ((uint64_t)lhi << 32) | llo;
      }
      if (lane == 0) prev = row_before;
      const bool has_prev = i > 0 && i < n;
      if (i < n) {
        if (k0[h] < kb || k0[h] >= ke) range = 1;
        if (has_prev && prev >= k0[h]) unsorted = 1;
      }
      if (i + 1 < n) {
        if (k1[h] < kb || k1[h] >= ke) range = 1;
        if (k0[h] >= k1[h]) unsorted = 1;
      }
    }
    if (chunk_ok && wbase < n) {
      // is this chunk's tile a stretch of the store (see above)?  Wave-uniform
      // (every key of the tile equal to K[lo + i - ta] IS the tile being the
      // stretch K[lo, lo + n_t): the window's end keys need no check; it must
      // be of this K, and the stretch inside it)
      const uint64_t ta = wbase / tileN * tileN;
      const uint64_t tb = ta + tileN < n ? ta + tileN : n;
      bool ok = e.gen == gen && (uint64_t)e.lo + (tb - ta) <= S;
      if (ok) {
        const uint64_t kbase = (uint64_t)e.lo - ta;  // K index of request key i: kbase + i (mod 2^64)
        bool mine = true;
#pragma unroll
        for (int h = 0; h < kRows; ++h) {
          const uint64_t i = wbase + (uint64_t)h * kRowKeys + 2 * (uint64_t)lane;
          if (i + 2 <= n && (e.lo & 1) == 0) {
            const u64x2 c = *reinterpret_cast<const u64x2*>(K + (kbase + i));
            mine = mine && c[0] == k0[h] && c[1] == k1[h];
          } else {
            if (i < n) mine = mine && K[kbase + i] == k0[h];
            if (i + 1 < n) mine = mine && K[kbase + i + 1] == k1[h];
          }
        }
        ok = __ballot(!mine) == 0;
      }
      // a chunk that is not marks its tile's word general for this request
      // (every such chunk writes the same word; one that is writes nothing): a
      // tile whose word is of another request is a stretch of the store
      if (lane == 0 && !ok) chunk_ok[wbase / tileN] = (int)(tile_tag(seq) | kTileGeneral);
    }
  }
  if (__ballot(range) && (threadIdx.x & 63) == 0) reject[kRejRange] = seq;
  if (__ballot(unsorted) && (threadIdx.x & 63) == 0) reject[kRejUnsorted] = seq;
}

// DENSE store addressed by explicit keys: the same request validation (keys
// strictly ascending, inside [kb, kb + cap)) before any slot is written.
__global__ __launch_bounds__(256) void k_validate_keys(const uint64_t* __restrict__ q, uint64_t n,
                                                       uint64_t kb, uint64_t cap, int* __restrict__ reject,
                                                       int seq, int* __restrict__ flags) {
  int range = 0, unsorted = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = q[i];
    if (i > 0 && q[i - 1] >= key) unsorted = 1;
    if (key < kb || key - kb >= cap) range = 1;
  }
  if (__ballot(range) && (threadIdx.x & 63) == 0) reject[kRejRange] = seq;
  if (__ballot(unsorted) && (threadIdx.x & 63) == 0) reject[kRejUnsorted] = seq;
  raise_flag(flags, F_RANGE, range != 0);
  raise_flag(flags, F_UNSORTED, unsorted != 0);
}

// Pass 2, fused with the request: k_resolve's search, then each lane applies
// the request to its (up to) 4 keys right away — store[slot] += val and/or
// out[i] = store[slot] — so the slots never go to HBM and back (28 B/key
// instead of 36: request key 8 + store key 8 + value 4 + store value 8).  An
// absent key is skipped (a pull reads 0, what its insertion gives); the flags
// tell the host to insert it and apply the request to it afterwards.
template <int NT>
__device__ __forceinline__ void stage_window(uint64_t* sK, const uint64_t* __restrict__ K, uint64_t lo,
                                             uint64_t W) {
  // straight to LDS (no VGPRs): each wave instruction moves 1 KiB of the
  // window; lanes past its end re-read its start (written, never read).  A
  // lane may read 8 B past K[S-1]: the key arrays carry kKeyPad spare elements
  // for it.
  const uint32_t nbytes = (uint32_t)W * 8u;
  const char* src = reinterpret_cast<const char*>(K + lo);
  for (uint32_t c = (threadIdx.x >> 6) * 1024u; c < nbytes; c += (NT / 64) * 1024u) {
    const uint32_t off = c + (threadIdx.x & 63) * 16u;
    const char* g = off < nbytes ? src + off : src;
    __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)((char*)sK + c), 16, 0, 0);
  }
}

// A lane's four slots as one word: p0 = its first key's place in the tile's
// window (13 bits: windows of at most 8192 keys), and bit d - 1 of the upper
// 19 for each further key d places after it (its keys are ascending, so d
// counts up; every further key within 19 places)
constexpr uint32_t kCodeBits = 13, kCodeReach = 19;
__device__ __forceinline__ void code_slots(uint32_t code, uint64_t lo, uint64_t* slot) {
  slot[0] = lo + (code & ((1u << kCodeBits) - 1));
  uint32_t m = code >> kCodeBits;
#pragma unroll
  for (int k = 1; k < kPerLane; ++k) {
    slot[k] = slot[0] + 1 + (uint64_t)__builtin_ctz(m | (1u << 31));
    m &= m - 1;
  }
}

// A coded tile's stretch of store values V[lo, hi) (4-B values) into LDS, from
// the 16-B aligned byte va0 <= 4 lo: whole 16-B chunks straight to LDS (as
// stage_window), the last partial chunk's values (at most 3) through VGPRs —
// nothing is read past 4 hi.  The caller waits (vmcnt) and meets the block.
template <int NT>
__device__ __forceinline__ void stage_vals(char* lds, const char* V, uint64_t va0, uint64_t vhi_b) {
  const uint32_t nfull = (uint32_t)((vhi_b - va0) & ~15ull);
  const char* src = V + va0;
  for (uint32_t c = (threadIdx.x >> 6) * 1024u; c < nfull; c += (NT / 64) * 1024u) {
    // (lanes past the whole chunks load nothing: their LDS bytes are the
    // tail's, written below)
    const uint32_t off = c + (threadIdx.x & 63) * 16u;
    if (off < nfull)
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + off),
                                       (__attribute__((address_space(3))) void*)(lds + c), 16, 0, 0);
  }
  const uint32_t tail = (uint32_t)(vhi_b - va0) - nfull;
  if (threadIdx.x * 4u < tail)
    *reinterpret_cast<uint32_t*>(lds + nfull + threadIdx.x * 4u) =
        *reinterpret_cast<const uint32_t*>(src + nfull + threadIdx.x * 4u);
}

// Pass 1 of a Push on trusted windows, coded form (PSG_RA_CODED): one 1024-thread
// block per 4096-key tile.  The request keys are validated as in
// k_validate_windows (strict ascent, the shard's range; reject words), and the
// tile is RESOLVED here, where they are read anyway, instead of in the apply:
//   - a window exactly as wide as the tile: its keys compared with K[lo + i]
//     (8 B / key of store keys) — a stretch;
//   - a wider one of at most 8192 keys: the lane codes cached for the tile
//     (with the key list's windows) are verified — the store key at each coded
//     place gathered and compared, 8 B per store key of the window — and if
//     they no longer place every key, the window is staged into LDS, every key
//     placed by an LDS search / gallop and, if every key is found and each
//     lane's keys fit one code, the new lane codes (4 B per 4 keys) written.
// k_resolve_apply<MI> then serves stretch and coded tiles from lo and the codes
// alone — no key re-read, no window, no search: a request that is a subset of
// its store's keys (a random 90 % of them, say) moves request key 8 + store
// keys 8 / density + code 2 + value 4 + store values 8 / density B per key, the
// general path 8 more (the request keys read twice).
__global__ __launch_bounds__(1024, 8) void k_validate_code(const uint64_t* __restrict__ q, uint64_t n,
                                                           const uint64_t* __restrict__ K, uint64_t S,
                                                           const Win* __restrict__ win, uint32_t gen, uint64_t kb,
                                                           uint64_t ke, int* __restrict__ reject, int seq, int vec,
                                                           uint32_t* __restrict__ tword,
                                                           uint32_t* __restrict__ codes,
                                                           uint64_t* __restrict__ learn) {
  constexpr int NT = 1024;
  constexpr uint64_t tileN = (uint64_t)NT * kPerLane;
  constexpr uint32_t winN = 2 * NT * kPerLane;
  __shared__ uint64_t sK[winN];
  __shared__ uint32_t s_bad[4];  // per tile, by parity: [verify, resolve]
  const uint64_t ntiles = (n + tileN - 1) / tileN;
  const int lane = threadIdx.x & 63;
  int range = 0, unsorted = 0;
  if (threadIdx.x < 4) s_bad[threadIdx.x] = 0;
  uint32_t it = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, ++it) {
    const uint64_t t0 = tile * tileN;
    const uint64_t t1 = (t0 + tileN < n) ? t0 + tileN : n;
    const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kPerLane;
    __syncthreads();  // the previous tile's readers are done with sK and the other flags
    if (threadIdx.x < 2) s_bad[((it + 1) & 1) * 2 + threadIdx.x] = 0;
    uint32_t* bad = &s_bad[(it & 1) * 2];
    // the tile's kind from its cached window alone (uniform)
    const Win e = win[tile];
    const bool cur = e.gen == gen && e.lo <= e.hi && (uint64_t)e.hi <= S;
    const uint64_t lo = e.lo, W = cur ? (uint64_t)(e.hi - e.lo) : 0;
    const uint64_t nk = t1 - t0;
    const bool stretch = cur && W == nk, coded = cur && W > nk && W <= winN;
    // a coded candidate's cached lane code, loaded beside the request keys
    uint32_t cc = 0;
    if (coded && i0 < t1) cc = codes[tile * NT + threadIdx.x];
    uint64_t key[kPerLane];
    if (i0 + kPerLane <= t1 && (vec & 1)) {
      const u64x2 a = *reinterpret_cast<const u64x2*>(q + i0);
      const u64x2 b = *reinterpret_cast<const u64x2*>(q + i0 + 2);
      key[0] = a[0];
      key[1] = a[1];
      key[2] = b[0];
      key[3] = b[1];
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) key[k] = i0 + k < t1 ? q[i0 + k] : 0;
    }
    // a learning request keeps the list it validates (the verified copy a
    // later request of this list is compared with, k_list_check)
    if (learn) {
      if (i0 + kPerLane <= t1) {
        reinterpret_cast<u64x2*>(learn + i0)[0] = u64x2{key[0], key[1]};
        reinterpret_cast<u64x2*>(learn + i0)[1] = u64x2{key[2], key[3]};
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          if (i0 + k < t1) learn[i0 + k] = key[k];
      }
    }
    // the store keys to compare with: a stretch tile's K[lo + i], a coded
    // candidate's at its code's places (gathered: the same lines of K)
    uint64_t sk[kPerLane] = {};
    uint64_t rel[kPerLane] = {};
    bool cok = true;
    const uint64_t kbase = lo + (i0 - t0);
    if (stretch) {
      if (i0 + kPerLane <= t1 && (kbase & 1) == 0) {
        const u64x2 a = *reinterpret_cast<const u64x2*>(K + kbase);
        const u64x2 b = *reinterpret_cast<const u64x2*>(K + kbase + 2);
        sk[0] = a[0];
        sk[1] = a[1];
        sk[2] = b[0];
        sk[3] = b[1];
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) sk[k] = i0 + k < t1 ? K[kbase + k] : 0;
      }
    } else if (coded) {
      code_slots(cc, 0, rel);
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        if (i0 + k >= t1) continue;
        if (rel[k] < W) sk[k] = K[lo + rel[k]];
        else cok = false;
      }
    }
    {
      // strict ascent against the key before this lane's four (the previous
      // lane's last by a shuffle; lane 0 of a wave loads it) and the range
      const uint64_t last = key[kPerLane - 1];
      const uint32_t plo = __shfl_up((uint32_t)last, 1, 64), phi = __shfl_up((uint32_t)(last >> 32), 1, 64);
      uint64_t prev = ((uint64_t)phi << 32) | plo;
      bool have_prev = true;
      if (lane == 0) {
        have_prev = i0 > 0 && i0 < t1;
        prev = have_prev ? q[i0 - 1] : 0;
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        if (i0 + k < t1) {
          if (key[k] < kb || key[k] >= ke) range = 1;
          if (have_prev && prev >= key[k]) unsorted = 1;
          prev = key[k];
          have_prev = true;
        }
      }
    }
    uint32_t st = kTileGeneral;
    if (stretch) {
      bool mine = true;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k)
        if (i0 + k < t1) mine = mine && sk[k] == key[k];
      if (__ballot(!mine) && lane == 0) bad[0] = 1;
      __syncthreads();
      st = bad[0] ? kTileGeneral : kTileStretch;
    } else if (coded) {
      // the codes cached for this tile still place every key (the steady
      // state of a repeated key list): K at each coded place is the key, the
      // first key at place 0 and the last at W - 1 (the window exactly the
      // tile's: a coded tile rewrites its whole stretch of values, which must
      // hold no other tile's keys)
      bool ok = cok;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        if (i0 + k >= t1) continue;
        ok = ok && sk[k] == key[k];
        if (i0 + k == t0) ok = ok && rel[k] == 0;
        if (i0 + k == t1 - 1) ok = ok && rel[k] == W - 1;
      }
      if (__ballot(!ok) && lane == 0) bad[0] = 1;
      __syncthreads();
      if (!bad[0]) {
        st = kTileCoded;
      } else {
        // no (valid) codes: resolve the tile in LDS and write them
        stage_window<NT>(sK, K, lo, W);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const uint32_t w = (uint32_t)W;
        uint32_t pos[kPerLane];
        ok = true;
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          pos[k] = 0;
          if (i0 + k >= t1) continue;
          const uint64_t kk = key[k];
          if (k == 0) {
            // with every key of the tile in its window, key i of the tile
            // sits in [i, i + W - n_t]: a search of that bracket (its misses
            // are tiles with absent keys, which are not coded anyway)
            const uint32_t ri = (uint32_t)(i0 - t0), a = ri < w ? ri : w;
            const uint32_t b = ri + (w - (uint32_t)nk) + 1 < w ? ri + (w - (uint32_t)nk) + 1 : w;
            r = a + lower_bound_lds(sK + a, b - a, kk);
          } else if (!(r < w && sK[r] >= kk)) {
            // gallop forward from the previous key's place (k_resolve_apply)
            uint32_t a = r < w ? r + 1 : w, b = a, step = 1;
            while (b < w && sK[b] < kk) {
              a = b + 1;
              b = a + step;
              step <<= 1;
            }
            if (b > w) b = w;
            if (a > b) a = b;
            r = a + lower_bound_lds(sK + a, b - a, kk);
          }
          ok = ok && r < w && sK[r] == kk;
          pos[k] = r;
        }
        if (i0 == t0) ok = ok && pos[0] == 0;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          if (i0 + k == t1 - 1) ok = ok && pos[k] == w - 1;
        uint32_t code = pos[0];
#pragma unroll
        for (int k = 1; k < kPerLane; ++k) {
          if (i0 + k >= t1) continue;
          const uint32_t d = pos[k] - pos[0];
          ok = ok && d >= 1 && d <= kCodeReach;
          if (ok) code |= 1u << (d - 1 + kCodeBits);
        }
        if (i0 < t1) codes[tile * NT + threadIdx.x] = code;
        if (__ballot(!ok) && lane == 0) bad[1] = 1;
        __syncthreads();
        st = bad[1] ? kTileGeneral : kTileCoded;
      }
    }
    if (threadIdx.x == 0) tword[tile] = tile_tag(seq) | st;
  }
  if (__ballot(range) && lane == 0) reject[kRejRange] = seq;
  if (__ballot(unsorted) && lane == 0) reject[kRejUnsorted] = seq;
}

// The validation of a Push whose key list is its verified copy (the lean
// apply's first pass instead of k_validate_code): the request keys compared
// with the copy a learning request of this list kept (k_validate_code's learn)
// — a plain two-stream compare, 16 B per key, instead of the store keys'
// lines at the coded places (8 / density) and the lane codes (1).  Keys equal
// to a list validated against this very K (its generation) are in range,
// ascending and at the places the cached windows and codes give, so each
// tile's word is its kind from its window alone: a stretch when the window is
// exactly the tile, else coded.  Any difference writes seq into
// rej[kRejList]: the lean apply then writes nothing and the host validates
// the request in full (W_NOTLIST).  One lane per 4 keys, grid-strided; the
// tile words by the lanes of each tile's first keys.
constexpr int kIdU = 2;  // groups of 4 keys in flight per lane (k_list_check, k_ident_check)

template <int NT>
__global__ __launch_bounds__(256) void k_list_check(const uint64_t* __restrict__ q,
                                                    const uint64_t* __restrict__ copy, uint64_t n,
                                                    const Win* __restrict__ win, uint32_t gen,
                                                    int* __restrict__ rej, int seq, int vec,
                                                    uint32_t* __restrict__ tword) {
  constexpr uint64_t tileN = 1024 * kPerLane;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  int bad = 0;
  // the tile words: one lane per tile
  const uint64_t ntiles = (n + tileN - 1) / tileN;
  for (uint64_t tile = gid; tile < ntiles; tile += stride) {
    const uint64_t i0 = tile * tileN;
    const uint64_t t1 = (i0 + tileN < n) ? i0 + tileN : n;
    const Win e = win[tile];
    const bool cur = e.gen == gen && e.lo <= e.hi;
    const uint64_t W = cur ? (uint64_t)(e.hi - e.lo) : 0;
    if (!cur || W < t1 - i0 || W > 2 * tileN) bad = 1;
    tword[tile] = tile_tag(seq) | (W == t1 - i0 ? kTileStretch : kTileCoded);
  }
  // the compare: groups of 4 keys (two 16-B loads of each array), kIdU groups
  // per lane in flight (k_ident_check's shape)
  uint64_t done = 0;
  if (vec) {
    const uint64_t ng = n / 4;
    done = ng * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * kBlock * kIdU + threadIdx.x; b < ng; b += stride * kIdU) {
      u64x2 a[kIdU][2], c[kIdU][2];
#pragma unroll
      for (int u = 0; u < kIdU; ++u) {
        const uint64_t j = b + (uint64_t)u * kBlock < ng ? b + (uint64_t)u * kBlock : b;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u64x2* pq = reinterpret_cast<const u64x2*>(q + 4 * j + 2 * h);
          const u64x2* pc = reinterpret_cast<const u64x2*>(copy + 4 * j + 2 * h);
          a[u][h] = NT ? __builtin_nontemporal_load(pq) : *pq;
          c[u][h] = NT ? __builtin_nontemporal_load(pc) : *pc;
        }
      }
#pragma unroll
      for (int u = 0; u < kIdU; ++u)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (a[u][h][0] != c[u][h][0] || a[u][h][1] != c[u][h][1]) bad = 1;
    }
  }
  for (uint64_t i = done + gid; i < n; i += stride)
    if (q[i] != copy[i]) bad = 1;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) rej[kRejList] = seq;
}

// The apply of a Push whose validation pass (k_validate_code) sorted its tiles,
// for the tiles that need no search: a stretch at slots lo + i, a coded tile at
// the places of its lane codes, its stretch of values staged into LDS, updated
// and written back whole (as k_resolve_apply<MI> does) — a kernel of its own,
// without the general path's window staging and search, so it keeps more in
// flight than the one instantiation that serves every kind.  Speculative, like
// the identity requests: the host sends a list here while its last attempt
// left no general tile; a general tile is left to k_resolve_apply<MI>, which
// the host launches as the follow-up (the word reports W_PARTIAL and raises
// kPending) and which then serves only the general tiles (vec bit 8).  (The
// tile words are only read here: each wave reads its tile's word itself.)
// 4-byte values.
template <int DT, int OP>
__global__ __launch_bounds__(1024, 8) void k_tile_apply(uint64_t n, const Win* __restrict__ win,
                                                        typename Elem<DT>::T* __restrict__ V,
                                                        const typename Elem<DT>::T* __restrict__ vals,
                                                        typename Elem<DT>::T* __restrict__ outv, int* __restrict__ rej,
                                                        int seq, int vec, Arrival arrival, uint32_t* __restrict__ word,
                                                        uint32_t tag_bits, const uint32_t* __restrict__ tword,
                                                        const uint32_t* __restrict__ codes) {
  using E = Elem<DT>;
  using T = typename E::T;
  static_assert(sizeof(T) == 4, "4-byte values");
  constexpr int NT = 1024;
  constexpr uint64_t tileN = (uint64_t)NT * kPerLane;
  __shared__ uint32_t sV[2 * NT * kPerLane + 8];  // a coded tile's values (windows of at most 8192 keys)
  __shared__ uint32_t s_cond;
  if (threadIdx.x == 0) s_cond = 0;
  __syncthreads();
  uint32_t uniform = rej[kPending] != 0 ? (uint32_t)W_GATED : 0u;
  if (rej[kRejRange] == seq) uniform |= W_RANGE;
  if (rej[kRejUnsorted] == seq) uniform |= W_UNSORTED;
  if (rej[kRejList] == seq) uniform |= W_NOTLIST;
  const uint64_t ntiles = uniform ? 0 : (n + tileN - 1) / tileN;
  const uint32_t tag = tile_tag(seq);
  int partial = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * tileN;
    const uint64_t t1 = (t0 + tileN < n) ? t0 + tileN : n;
    const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kPerLane;
    const uint32_t tw = tword[tile];
    const uint32_t st = (tw >> 2) == (tag >> 2) ? (tw & 3u) : kTileGeneral;
    if (st != kTileStretch && st != kTileCoded) {  // (uniform) the follow-up's
      partial = 1;
      continue;
    }
    const Win e = win[tile];
    const uint64_t lo = e.lo;
    const bool whole = i0 + kPerLane <= t1;
    T v[kPerLane];
    if (whole && (vec & 1)) {
      const f32x4 x = __builtin_bit_cast(f32x4, ((vec & 16) ? *reinterpret_cast<const u32x4*>(vals + i0) : __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vals + i0))));
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) v[k] = x[k];
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) v[k] = i0 + k < t1 ? vals[i0 + k] : (T)0.0f;
    }
    T o[kPerLane];
    if (st == kTileStretch) {
      const uint64_t s0 = lo + (i0 - t0);
      if (whole && (s0 & 3) == 0) {
        f32x4 x = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(V + s0));
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          o[k] = E::add1(x[k], v[k]);
          x[k] = o[k];
        }
        *reinterpret_cast<u32x4*>(V + s0) = __builtin_bit_cast(u32x4, x);
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          o[k] = (T)0.0f;
          if (i0 + k < t1) {
            o[k] = E::add1(V[s0 + k], v[k]);
            V[s0 + k] = o[k];
          }
        }
      }
    } else {
      // the tile's stretch of values V[lo, hi) in LDS from the 16-B aligned
      // byte va0, updated at the coded places, written back whole
      uint64_t slot[kPerLane];
      code_slots(codes[tile * NT + threadIdx.x], lo, slot);
      const uint64_t vlo_b = lo * 4, vhi_b = (uint64_t)e.hi * 4, va0 = vlo_b & ~15ull;
      char* lds = reinterpret_cast<char*>(sV);
      stage_vals<NT>(lds, reinterpret_cast<const char*>(V), va0, vhi_b);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      T* sv = reinterpret_cast<T*>(lds + (vlo_b - va0));
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        o[k] = (T)0.0f;
        if (i0 + k < t1) {
          o[k] = E::add1(sv[slot[k] - lo], v[k]);
          sv[slot[k] - lo] = o[k];
        }
      }
      __syncthreads();
      const uint32_t nbytes = (uint32_t)(vhi_b - va0);
      char* Vb = reinterpret_cast<char*>(V);
      for (uint32_t c = threadIdx.x * 16u; c < nbytes; c += NT * 16u) {
        const uint64_t gb = va0 + c;
        if (gb >= vlo_b && c + 16u <= nbytes) {
          *reinterpret_cast<u32x4*>(Vb + gb) = *reinterpret_cast<const u32x4*>(lds + c);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint64_t b = gb + 4u * j;
            if (b >= vlo_b && b < vhi_b)
              *reinterpret_cast<uint32_t*>(Vb + b) = *reinterpret_cast<const uint32_t*>(lds + c + 4u * j);
          }
        }
      }
      __syncthreads();  // the next tile stages into sV
    }
    if constexpr ((OP & PSG_PULL) != 0) {
      if (whole && (vec & 1)) {
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, f32x4{o[0], o[1], o[2], o[3]}),
                                    reinterpret_cast<u32x4*>(outv + i0));
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          if (i0 + k < t1) outv[i0 + k] = o[k];
      }
    }
  }
  const uint64_t after = block_arrive(partial ? 2u : 0u, &s_cond, arrival);
  request_done(after, arrival, uniform, rej + kPending, word, tag_bits, W_PARTIAL);
}

// The whole 16-B chunks of a coded tile's values (stage_vals' DMA half), issued
// a tile ahead by k_tile_apply_db.
template <int NT>
__device__ __forceinline__ void stage_chunks(char* lds, const char* V, uint64_t va0, uint64_t vhi_b) {
  const uint32_t nfull = (uint32_t)((vhi_b - va0) & ~15ull);
  const char* src = V + va0;
  for (uint32_t c = (threadIdx.x >> 6) * 1024u; c < nfull; c += (NT / 64) * 1024u) {
    const uint32_t off = c + (threadIdx.x & 63) * 16u;
    if (off < nfull)
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + off),
                                       (__attribute__((address_space(3))) void*)(lds + c), 16, 0, 0);
  }
}

// A block barrier for LDS alone: this wave's LDS accesses done, then the
// barrier — without __syncthreads()'s fence, which would also wait for every
// global access in flight (the next tile's staging among them)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

constexpr uint32_t kTaBuf = 2 * 1024 * kPerLane * 4 + 32;  // bytes: a window of at most 8192 values + alignment
__shared__ __attribute__((aligned(16))) char ta_buf0[kTaBuf];
__shared__ __attribute__((aligned(16))) char ta_buf1[kTaBuf];

// One tile of k_tile_apply_db, its window (if coded) in ta_buf<B>, staging the
// block's next tile into the other buffer meanwhile.
template <int DT, int OP, int B>
__device__ __forceinline__ void tile_apply_step(uint64_t tile, uint64_t n, uint64_t ntiles, const Win* __restrict__ win,
                                                typename Elem<DT>::T* __restrict__ V,
                                                const typename Elem<DT>::T* __restrict__ vals,
                                                typename Elem<DT>::T* __restrict__ outv, int vec, uint32_t tag,
                                                const uint32_t* __restrict__ tword,
                                                const uint32_t* __restrict__ codes, int& partial) {
  using E = Elem<DT>;
  using T = typename E::T;
  constexpr int NT = 1024;
  constexpr uint64_t tileN = (uint64_t)NT * kPerLane;
  char* const lds = B ? ta_buf1 : ta_buf0;
  char* const other = B ? ta_buf0 : ta_buf1;
  const char* Vc = reinterpret_cast<const char*>(V);
  auto kind = [&](uint64_t t) -> uint32_t {
    const uint32_t tw = tword[t];
    return (tw >> 2) == (tag >> 2) ? (tw & 3u) : (uint32_t)kTileGeneral;
  };
  const uint64_t next = tile + gridDim.x;
  const bool next_coded = next < ntiles && kind(next) == kTileCoded;
  auto stage_next = [&]() {
    if (next_coded) {
      const Win e2 = win[next];
      stage_chunks<NT>(other, Vc, ((uint64_t)e2.lo * 4) & ~15ull, (uint64_t)e2.hi * 4);
    }
  };
  const uint32_t st = kind(tile);
  if (st != kTileStretch && st != kTileCoded) {  // (uniform) the follow-up's
    partial = 1;
    stage_next();
    return;
  }
  const uint64_t t0 = tile * tileN;
  const uint64_t t1 = (t0 + tileN < n) ? t0 + tileN : n;
  const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kPerLane;
  const Win e = win[tile];
  const uint64_t lo = e.lo;
  const bool whole = i0 + kPerLane <= t1;
  T v[kPerLane];
  if (whole && (vec & 1)) {
    const f32x4 x = __builtin_bit_cast(f32x4, ((vec & 16) ? *reinterpret_cast<const u32x4*>(vals + i0) : __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vals + i0))));
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) v[k] = x[k];
  } else {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) v[k] = i0 + k < t1 ? vals[i0 + k] : (T)0.0f;
  }
  T o[kPerLane];
  if (st == kTileStretch) {
    // done in registers before the next tile's staging is issued (a load
    // after it would wait for it)
    const uint64_t s0 = lo + (i0 - t0);
    if (whole && (s0 & 3) == 0) {
      f32x4 x = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(V + s0));
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        o[k] = E::add1(x[k], v[k]);
        x[k] = o[k];
      }
      *reinterpret_cast<u32x4*>(V + s0) = __builtin_bit_cast(u32x4, x);
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        o[k] = (T)0.0f;
        if (i0 + k < t1) {
          o[k] = E::add1(V[s0 + k], v[k]);
          V[s0 + k] = o[k];
        }
      }
    }
    stage_next();
  } else {
    // this tile's code, values and last partial chunk, all landed (with the
    // chunks staged a round ago, issued before them) before the next tile's
    // staging goes out
    const uint64_t vlo_b = lo * 4, vhi_b = (uint64_t)e.hi * 4, va0 = vlo_b & ~15ull;
    const uint32_t nfull = (uint32_t)((vhi_b - va0) & ~15ull);
    const uint32_t tail = (uint32_t)(vhi_b - va0) - nfull;
    const uint32_t code = codes[tile * NT + threadIdx.x];
    uint32_t tailv = 0;
    if (threadIdx.x * 4u < tail) tailv = *reinterpret_cast<const uint32_t*>(Vc + va0 + nfull + threadIdx.x * 4u);
    asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(code), "v"(tailv));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_next();
    uint64_t slot[kPerLane];
    code_slots(code, lo, slot);
    if (threadIdx.x * 4u < tail) *reinterpret_cast<uint32_t*>(lds + nfull + threadIdx.x * 4u) = tailv;
    lds_barrier();
    T* sv = reinterpret_cast<T*>(lds + (vlo_b - va0));
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      o[k] = (T)0.0f;
      if (i0 + k < t1) {
        o[k] = E::add1(sv[slot[k] - lo], v[k]);
        sv[slot[k] - lo] = o[k];
      }
    }
    lds_barrier();
    const uint32_t nbytes = (uint32_t)(vhi_b - va0);
    char* Vb = reinterpret_cast<char*>(V);
    for (uint32_t c = threadIdx.x * 16u; c < nbytes; c += NT * 16u) {
      const uint64_t gb = va0 + c;
      if (gb >= vlo_b && c + 16u <= nbytes) {
        *reinterpret_cast<u32x4*>(Vb + gb) = *reinterpret_cast<const u32x4*>(lds + c);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint64_t bb = gb + 4u * j;
          if (bb >= vlo_b && bb < vhi_b)
            *reinterpret_cast<uint32_t*>(Vb + bb) = *reinterpret_cast<const uint32_t*>(lds + c + 4u * j);
        }
      }
    }
    lds_barrier();  // this buffer read out before the round after next stages into it
  }
  if constexpr ((OP & PSG_PULL) != 0) {
    if (whole && (vec & 1)) {
      __builtin_nontemporal_store(__builtin_bit_cast(u32x4, f32x4{o[0], o[1], o[2], o[3]}),
                                  reinterpret_cast<u32x4*>(outv + i0));
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k)
        if (i0 + k < t1) outv[i0 + k] = o[k];
    }
  }
}

// k_tile_apply with the coded tiles' values staged a tile ahead: while a block
// updates and writes back tile t's stretch of values from one LDS buffer, the
// DMA of its next tile's (t + grid) fills the other — a block keeps two
// windows in flight instead of one (128 KiB of LDS per CU at two blocks).
// Tile windows are disjoint (k_validate_code's exactness: a coded tile's
// first key at place 0, its last at W - 1), so staging the next before this
// one is written back reads no value this kernel writes — but for the up to
// 3 values before lo that the 16-B alignment stages and the write-back skips.
// The last partial chunk (at most 3 values) is read through VGPRs in the
// tile's own round, as stage_vals does.  The block's tiles alternate between
// the two buffers (two static arrays: the compiler sees that the LDS accesses
// of one tile cannot alias the other's staging, and waits for nothing of it).
// (PSG_TA_DB=0: k_tile_apply, A/B.)
template <int DT, int OP>
__global__ __launch_bounds__(1024, 8) void k_tile_apply_db(uint64_t n, const Win* __restrict__ win,
                                                           typename Elem<DT>::T* __restrict__ V,
                                                           const typename Elem<DT>::T* __restrict__ vals,
                                                           typename Elem<DT>::T* __restrict__ outv,
                                                           int* __restrict__ rej, int seq, int vec, Arrival arrival,
                                                           uint32_t* __restrict__ word, uint32_t tag_bits,
                                                           const uint32_t* __restrict__ tword,
                                                           const uint32_t* __restrict__ codes) {
  static_assert(sizeof(typename Elem<DT>::T) == 4, "4-byte values");
  constexpr uint64_t tileN = 1024 * kPerLane;
  __shared__ uint32_t s_cond;
  if (threadIdx.x == 0) s_cond = 0;
  __syncthreads();
  uint32_t uniform = rej[kPending] != 0 ? (uint32_t)W_GATED : 0u;
  if (rej[kRejRange] == seq) uniform |= W_RANGE;
  if (rej[kRejUnsorted] == seq) uniform |= W_UNSORTED;
  if (rej[kRejList] == seq) uniform |= W_NOTLIST;
  const uint64_t ntiles = uniform ? 0 : (n + tileN - 1) / tileN;
  const uint32_t tag = tile_tag(seq);
  // the first tile's chunks
  if (blockIdx.x < ntiles) {
    const uint32_t tw = tword[blockIdx.x];
    if ((tw >> 2) == (tag >> 2) && (tw & 3u) == kTileCoded) {
      const Win e = win[blockIdx.x];
      stage_chunks<1024>(ta_buf0, reinterpret_cast<const char*>(V), ((uint64_t)e.lo * 4) & ~15ull,
                         (uint64_t)e.hi * 4);
    }
  }
  int partial = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += 2 * (uint64_t)gridDim.x) {
    tile_apply_step<DT, OP, 0>(tile, n, ntiles, win, V, vals, outv, vec, tag, tword, codes, partial);
    if (tile + gridDim.x < ntiles)
      tile_apply_step<DT, OP, 1>(tile + gridDim.x, n, ntiles, win, V, vals, outv, vec, tag, tword, codes, partial);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (no staging left in flight)
  __syncthreads();
  const uint64_t after = block_arrive(partial ? 2u : 0u, &s_cond, arrival);
  request_done(after, arrival, uniform, rej + kPending, word, tag_bits, W_PARTIAL);
}

// __launch_bounds__(NT, 8): 8 waves per SIMD, i.e. two 1024-thread blocks per
// CU (the LDS holds two 64 KiB windows).  Without the bound the Pull
// instantiation used 91 SGPRs (97 with VCC and the rest): one block per CU,
// and the 10 M-key Pull took 56 us instead of 40.
// MI: the stretch-tile form (chunk_ok, §3.1 of DESIGN.md) — a separate
// instantiation, so the kernels that never see a stretch tile (sparse tiles,
// Pulls) keep their registers.
template <int DT, int OP, int NT, bool SP = false, int WM = 2, bool MI = false>
__global__ __launch_bounds__(NT, (WM == 2 ? 8 : 4)) void k_resolve_apply(const uint64_t* __restrict__ q, uint64_t n,
                                                       const uint64_t* __restrict__ K, uint64_t S,
                                                       Win* __restrict__ win, uint32_t gen, uint64_t kb,
                                                       uint64_t ke,
                                                       typename Elem<DT>::T* __restrict__ V,
                                                       const typename Elem<DT>::T* __restrict__ vals,
                                                       typename Elem<DT>::T* __restrict__ outv,
                                                       int* __restrict__ rej, int seq, int vec,
                                                       Arrival arrival, uint32_t* __restrict__ word,
                                                       uint32_t tag_bits, const uint32_t* __restrict__ tword,
                                                       const uint32_t* __restrict__ codes) {
  using E = Elem<DT>;
  using T = typename E::T;
  constexpr uint64_t tileN = (uint64_t)NT * kPerLane;  // request keys per block tile
  // LDS window of store keys: WM times the tile (2; 4 for a request at most
  // 2 in 5 of whose store's keys it asks for, whose windows would otherwise
  // stream through LDS in chunks)
  constexpr uint32_t winN = WM * NT * kPerLane;
  __shared__ uint64_t sK[winN];
  __shared__ uint64_t sBound[2];
  __shared__ uint32_t s_cond;
  // A request that writes the store was validated as a whole first: if
  // k_validate_windows rejected it, write nothing (every block skips its
  // tiles, uniformly, before any store access, and still signals).  A Pull
  // writes only its reply, so it checks its keys here, in the same pass
  // (CHECK), and the host rejects it from its word before anything else
  // happens (no insert of absent keys).  A request behind one that awaits
  // the host's follow-up (kPending) is gated: it writes nothing either.
  constexpr bool CHECK = OP == PSG_PULL;
  if (threadIdx.x == 0) s_cond = 0;
  __syncthreads();
  uint32_t uniform = rej[kPending] != 0 ? (uint32_t)W_GATED : 0u;
  if constexpr (!CHECK) {
    if (rej[kRejRange] == seq) uniform |= W_RANGE;
    if (rej[kRejUnsorted] == seq) uniform |= W_UNSORTED;
  }
  const bool skip = uniform != 0;
  int missing = 0, range = 0, unsorted = 0, winmiss = 0;
  uint64_t after = 0;
  bool arrived = false;
  const uint64_t ntiles = skip ? 0 : (n + tileN - 1) / tileN;
  // A tile's inputs that do not depend on its window — its window entry, its
  // request keys, the key before a wave's first (CHECK) and (Push) its values
  // — are loaded one tile ahead (pf), while the current tile's store values
  // are in flight: a tile then waits on two dependent HBM round trips (its
  // window, then its store values) instead of three (entry, window, values).
  uint64_t nkey[kPerLane] = {}, nprev = 0, nqfirst = 0, nqlast = 0;
  T nv[kPerLane] = {};
  uint32_t ncode = 0;
  Win ne = {};
  // a tile the validation pass found to be a stretch of the store (no chunk
  // of it marked with this request's seq, k_validate_windows): served at
  // slots lo + i, its keys not loaded again (block-uniform; carried in the
  // window entry's spare word, ne.pad)
  auto load_tile = [&](uint64_t tl) {
    const uint64_t a0 = tl * tileN;
    const uint64_t a1 = (a0 + tileN < n) ? a0 + tileN : n;
    const uint64_t j0 = a0 + (uint64_t)threadIdx.x * kPerLane;
    ne = win[tl];
    ne.pad = kTileGeneral;
    if constexpr (MI && !CHECK) {
      const uint32_t tw = tword[tl];
      ne.pad = (tw >> 2) == (tile_tag(seq) >> 2) ? (tw & 3u) : kTileStretch;
      // (vec bit 8: the follow-up of a k_tile_apply, which served every
      // stretch and coded tile already: those run as tiles of no keys)
      if ((vec & 8) && ne.pad != kTileGeneral) ne.pad = kTileDone;
      if (ne.pad == kTileCoded) ncode = codes[tl * NT + threadIdx.x];
    }
    if (ne.pad) {
      nqfirst = ne.first;
      nqlast = ne.last;
    } else {
    nqfirst = q[a0];
    nqlast = q[a1 - 1];
    if (j0 + kPerLane <= a1 && (vec & 2)) {
      const u64x2 a = *reinterpret_cast<const u64x2*>(q + j0);
      const u64x2 b = *reinterpret_cast<const u64x2*>(q + j0 + 2);
      nkey[0] = a[0];
      nkey[1] = a[1];
      nkey[2] = b[0];
      nkey[3] = b[1];
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) nkey[k] = j0 + k < a1 ? q[j0 + k] : 0;
    }
    if constexpr (CHECK) nprev = ((threadIdx.x & 63) == 0 && j0 > 0 && j0 < a1) ? q[j0 - 1] : 0;
    }
    if constexpr ((OP & PSG_PUSH) != 0) {
      bool vdone = false;
      if constexpr (sizeof(T) == 4) {
        if (j0 + kPerLane <= a1 && (vec & 1)) {
          const f32x4 x = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(vals + j0));
#pragma unroll
          for (int k = 0; k < kPerLane; ++k) nv[k] = x[k];
          vdone = true;
        }
      }
      if (!vdone) {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) nv[k] = (j0 + k < a1) ? vals[j0 + k] : (T)0.0f;
      }
    }
  };
  if (blockIdx.x < ntiles) load_tile(blockIdx.x);
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * tileN;
    // the window cached for this tile, staged speculatively: it is right when
    // it was computed against this K for this tile's first and last key
    // (checked below)
    const Win e = ne;
    // (MI) a tile k_tile_apply served already runs as a stretch tile of no
    // keys (uniform): nothing read or written, the next tile still prefetched
    const uint64_t t1 = MI && e.pad == kTileDone ? t0 : ((t0 + tileN < n) ? t0 + tileN : n);
    const bool ident = MI && e.pad != 0;
    const bool cur = e.gen == gen;
    uint64_t lo = cur ? e.lo : 0, hi = cur ? e.hi : 0;
    if (hi > S) hi = S;
    if (hi < lo) hi = lo;  // unsorted input
    uint64_t W = hi - lo;
    bool staged = W <= (uint64_t)winN;
    const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kPerLane;
    const bool whole = i0 + kPerLane <= t1;
    if (!ident && cur && staged) stage_window<NT>(sK, K, lo, W);
    // a coded tile (4-B values): its stretch of store values V[lo, hi) is
    // staged into LDS, updated there at the coded places and written back
    // whole — 16-B accesses to HBM where the places themselves are scattered
    // (a random subset of the store).  The tile windows of one request are
    // disjoint, so the slots between its keys are rewritten unchanged by the
    // only block that touches them.
    bool cv = false;
    uint64_t vlo_b = 0, vhi_b = 0, va0 = 0;
    if constexpr (MI && sizeof(T) == 4) {
      cv = e.pad == kTileCoded;
      vlo_b = lo * 4;
      vhi_b = (uint64_t)e.hi * 4;
      va0 = vlo_b & ~15ull;
      if (cv) stage_vals<NT>(reinterpret_cast<char*>(sK), reinterpret_cast<const char*>(V), va0, vhi_b);
    }
    const uint64_t qfirst = nqfirst, qlast = nqlast;
    uint64_t key[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) key[k] = nkey[k];
    if constexpr (CHECK) {
      // strict ascent against the key before this lane's four (the previous
      // lane's last, by a shuffle; lane 0 of a wave loads it) and the range
      const uint64_t last = key[kPerLane - 1];
      const uint32_t plo = __shfl_up((uint32_t)last, 1, 64), phi = __shfl_up((uint32_t)(last >> 32), 1, 64);
      uint64_t prev = ((uint64_t)phi << 32) | plo;
      bool have_prev = true;
      if ((threadIdx.x & 63) == 0) {
        have_prev = i0 > 0 && i0 < t1;
        prev = nprev;
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        if (i0 + k < t1) {
          if (key[k] < kb || key[k] >= ke) range = 1;
          if (have_prev && prev >= key[k]) unsorted = 1;
          prev = key[k];
          have_prev = true;
        }
      }
    }
    T v[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) v[k] = nv[k];
    const uint32_t code = ncode;
    // The window reaches LDS by DMA (global_load_lds), which only vmcnt
    // tracks; the barrier's workgroup fence does not wait on it in
    // non-tgsplit mode.  Wait explicitly so no wave reads another wave's part
    // of the window before it has landed.  (A stretch tile stages nothing: it
    // neither waits for the loads in flight — the next tile's, prefetched —
    // nor meets the other waves; block-uniform.)
    if (!ident || cv) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (!ident && !(cur && e.first == qfirst && e.last == qlast)) {
      // stale or absent window (block-uniform): search both ends (waves 0 and
      // 1), keep the result for the next request on these keys, restage
      const int wv = threadIdx.x >> 6;
      if (wv < 2) {
        const uint64_t r = lower_bound_wave(K, S, wv == 0 ? qfirst : qlast);
        if ((threadIdx.x & 63) == 0) sBound[wv] = r;
      }
      __syncthreads();
      lo = sBound[0];
      hi = sBound[1] < S ? sBound[1] + 1 : S;
      if (hi < lo) hi = lo;
      W = hi - lo;
      staged = W <= (uint64_t)winN;
      if (threadIdx.x == 0) {
        win[tile].first = qfirst;
        win[tile].last = qlast;
        win[tile].lo = (uint32_t)lo;
        win[tile].hi = (uint32_t)hi;
        win[tile].gen = gen;
      }
      if (staged) stage_window<NT>(sK, K, lo, W);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      winmiss = 1;
    }
    uint32_t r = 0;
    uint64_t slot[kPerLane];
    bool hit[kPerLane];
    if (ident) {
      // key i of the tile is K[lo + i - t0] (a stretch), or at the places its
      // lane's code gives (a coded tile), as the validation pass found
      if (e.pad == kTileCoded) {
        code_slots(code, lo, slot);
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) slot[k] = lo + (i0 + k - t0);
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) hit[k] = i0 + k < t1;
    } else if (staged) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const uint64_t i = i0 + k;
        hit[k] = false;
        slot[k] = 0;
        if (i >= t1) continue;
        const uint64_t kk = key[k];
        const uint32_t w = (uint32_t)W;
        if (k == 0) {
          r = lower_bound_lds(sK, w, kk);
        } else if (!(r < w && sK[r] >= kk)) {
          // gallop forward from the previous key's place (probes at +1, +2,
          // +4, ... then a search of the last gap): the next store key for a
          // request that covers its stretch of the store, two or three probes
          // for one that asks for every other or every third key — where a
          // search of the whole rest of the window took ~13 dependent LDS reads
          // (r == w: the previous key is past the window, and so is this one)
          uint32_t a = r < w ? r + 1 : w, b = a, step = 1;  // sK[a - 1] < kk
          while (b < w && sK[b] < kk) {
            a = b + 1;
            b = a + step;
            step <<= 1;
          }
          if (b > w) b = w;
          if (a > b) a = b;  // (a <= w always; kept explicit: b - a is a count)
          r = a + lower_bound_lds(sK + a, b - a, kk);
        }
        const bool found = r < w && sK[r] == kk;
        hit[k] = found;
        slot[k] = lo + r;
        if (!found) missing++;
      }
    } else if (W <= 16 * (uint64_t)winN) {
      // The window is larger than the LDS holds: a request sparse in the store
      // (the store holds more keys than the tile asks for — every other key,
      // say).  Both the tile's keys and the window ascend, so the window
      // streams through LDS in winN-key chunks and chunk c places exactly the
      // keys between its first and last store key: the window is read once,
      // where a search per key in HBM made dependent round trips per key
      // (2.4x the kernel time at every other key).  Block-uniform loop.
      bool open[kPerLane];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        hit[k] = false;
        slot[k] = 0;
        open[k] = i0 + k < t1;
      }
      for (uint64_t c0 = lo; c0 < hi; c0 += winN) {
        const uint32_t wc = (uint32_t)(hi - c0 < (uint64_t)winN ? hi - c0 : (uint64_t)winN);
        __syncthreads();  // the previous chunk's readers are done with sK
        stage_window<NT>(sK, K, c0, wc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const uint64_t clast = sK[wc - 1];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          if (open[k] && key[k] <= clast) {
            const uint32_t rc = lower_bound_lds(sK, wc, key[k]);
            hit[k] = sK[rc] == key[k];
            slot[k] = c0 + rc;
            open[k] = false;
          }
        }
        if (clast >= qlast) break;  // every key of the tile placed (uniform)
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k)
        if (i0 + k < t1 && !hit[k]) missing++;  // (keys past the window's end: absent)
    } else {
      // sparser still (under one key in 32 of the window): a search per key
      // in HBM reads less than the window would
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        hit[k] = false;
        slot[k] = 0;
        if (i0 + k >= t1) continue;
        const uint64_t p = lower_bound_dev(K, lo, hi, key[k]);
        hit[k] = p < S && K[p] == key[k];
        slot[k] = p;
        if (!hit[k]) missing++;
      }
    }
    if (tile + gridDim.x >= ntiles) {  // this block's last tile (uniform)
      after = block_arrive((missing ? 1u : 0u) | (winmiss ? 2u : 0u) | (range ? 4u : 0u) | (unsorted ? 8u : 0u),
                           &s_cond, arrival);
      arrived = true;
    }
    // apply.  A lane whose 4 keys are 4 consecutive, 16-B aligned store
    // slots (the common case: a request that covers a stretch of the store)
    // moves its store values as one vector; request values and replies are one
    // vector when T is 4 B, the tile is whole and the caller's arrays are 16-B
    // aligned (vec & 1, checked on the host)
    T o[kPerLane], x[kPerLane];
    bool vecv = false;
    if constexpr (sizeof(T) == 4)
      vecv = hit[0] && hit[1] && hit[2] && hit[3] && slot[3] == slot[0] + 3 && (slot[0] & 3) == 0;
    // (vec & 4, a Push sparse in its store) a lane whose 4 keys lie in one
    // 32-B aligned span of 8 slots that no other lane writes — its wave
    // neighbours' keys outside it, and not at a wave's edge, whose neighbour
    // is another wave's — moves the span as two vectors and writes it back
    // whole, its other slots unchanged: every line written in full
    bool span8 = false;
    uint64_t sbase = 0;
    f32x4 sa = {}, sb = {};
    if constexpr (SP && sizeof(T) == 4 && (OP & PSG_PUSH) != 0) {
      {
        // a neighbour bounds the span only through its key next to this
        // lane's, found: a lane whose key there is absent says nothing about
        // where the found keys of the lanes beyond it sit (they may fall in
        // the span), so it disables the span (its first slot reads 0 for the
        // lane before it, its last all ones for the lane after)
        const uint64_t lo_hit = hit[0] ? slot[0] : 0ull;
        const uint64_t hi_hit = hit[3] ? slot[3] : ~0ull;
        const uint32_t plo = __shfl_up((uint32_t)hi_hit, 1, 64), phi = __shfl_up((uint32_t)(hi_hit >> 32), 1, 64);
        const uint32_t nlo = __shfl_down((uint32_t)lo_hit, 1, 64), nhi = __shfl_down((uint32_t)(lo_hit >> 32), 1, 64);
        const uint64_t prev_hi = ((uint64_t)phi << 32) | plo, next_lo = ((uint64_t)nhi << 32) | nlo;
        const int lane = threadIdx.x & 63;
        sbase = slot[0] & ~7ull;
        span8 = !vecv && lane != 0 && lane != 63 && hit[0] && hit[1] && hit[2] && hit[3] && slot[3] < sbase + 8 &&
                sbase + 8 <= S && prev_hi < sbase && next_lo >= sbase + 8;
      }
    }
    if (cv) {
      if constexpr (MI && sizeof(T) == 4) {
        const T* sV = reinterpret_cast<const T*>(reinterpret_cast<const char*>(sK) + (vlo_b - va0));
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) x[k] = hit[k] ? sV[slot[k] - lo] : (T)0.0f;
      }
    } else if (span8) {
      if constexpr (sizeof(T) == 4 && (OP & PSG_PUSH) != 0) {
        sa = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(V + sbase));
        sb = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(V + sbase + 4));
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          const uint32_t d = (uint32_t)(slot[k] - sbase);
          T y = sa[0];
#pragma unroll
          for (int e = 1; e < 8; ++e)
            if (d == (uint32_t)e) y = e < 4 ? sa[e & 3] : sb[e & 3];
          x[k] = y;
        }
      }
    } else if (vecv) {
      if constexpr (sizeof(T) == 4) {
        const f32x4 xv = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(V + slot[0]));
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) x[k] = xv[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) x[k] = hit[k] ? V[slot[k]] : (T)0.0f;
    }
    // the next tile's inputs, issued behind this tile's store values (whose
    // waits then leave them in flight)
    if (tile + gridDim.x < ntiles) load_tile(tile + gridDim.x);
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      o[k] = x[k];
      if constexpr ((OP & PSG_PUSH) != 0) o[k] = E::add1(x[k], v[k]);
    }
    if constexpr ((OP & PSG_PUSH) != 0) {
      if (cv) {
        if constexpr (MI && sizeof(T) == 4) {
          T* sV = reinterpret_cast<T*>(reinterpret_cast<char*>(sK) + (vlo_b - va0));
#pragma unroll
          for (int k = 0; k < kPerLane; ++k)
            if (hit[k]) sV[slot[k] - lo] = o[k];
          __syncthreads();
          // write the stretch back: whole 16-B chunks inside [lo, hi) as
          // vectors, the partial first and last chunks value by value
          const uint32_t nbytes = (uint32_t)(vhi_b - va0);
          char* Vb = reinterpret_cast<char*>(V);
          const char* sb = reinterpret_cast<const char*>(sK);
          for (uint32_t c = threadIdx.x * 16u; c < nbytes; c += NT * 16u) {
            const uint64_t gb = va0 + c;
            if (gb >= vlo_b && c + 16u <= nbytes) {
              *reinterpret_cast<u32x4*>(Vb + gb) = *reinterpret_cast<const u32x4*>(sb + c);
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const uint64_t b = gb + 4u * j;
                if (b >= vlo_b && b < vhi_b)
                  *reinterpret_cast<uint32_t*>(Vb + b) = *reinterpret_cast<const uint32_t*>(sb + c + 4u * j);
              }
            }
          }
        }
      } else if (span8) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
          for (int k = 0; k < kPerLane; ++k) {
            const uint32_t d = (uint32_t)(slot[k] - sbase);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (d == (uint32_t)e) {
                if (e < 4) sa[e & 3] = o[k];
                else sb[e & 3] = o[k];
              }
          }
          *reinterpret_cast<u32x4*>(V + sbase) = __builtin_bit_cast(u32x4, sa);
          *reinterpret_cast<u32x4*>(V + sbase + 4) = __builtin_bit_cast(u32x4, sb);
        }
      } else if (vecv) {
        if constexpr (sizeof(T) == 4)
          *reinterpret_cast<u32x4*>(V + slot[0]) = __builtin_bit_cast(u32x4, f32x4{o[0], o[1], o[2], o[3]});
      } else {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          if (hit[k]) V[slot[k]] = o[k];
      }
    }
    if constexpr ((OP & PSG_PULL) != 0) {
      bool done = false;
      if constexpr (sizeof(T) == 4) {
        if (whole && (vec & 1)) {
          *reinterpret_cast<u32x4*>(outv + i0) = __builtin_bit_cast(u32x4, f32x4{o[0], o[1], o[2], o[3]});
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          if (i0 + k < t1) outv[i0 + k] = o[k];
      }
    }
    // the next tile may restage sK: every wave is done reading this one's
    // (a stretch tile read none)
    if (!ident || cv) __syncthreads();
  }
  if (!arrived) after = block_arrive(0u, &s_cond, arrival);  // no tile (rejected, gated, or a spare block)
  request_done(after, arrival, uniform, rej + kPending, word, tag_bits);
}

// ---- identity requests ------------------------------------------------------
// A request whose keys are exactly a stretch of the store's key array,
// q[i] == K[D + i] for every i < n, needs no search and no window in LDS: key i
// is at slot D + i.  That is a key list covering its range of the store — the
// steady state of a list repeated against a store that holds it (configs[3],
// where every worker pushes the shard's whole list).  D = lower_bound(K, q[0])
// is the lower end of the first tile's window, cached for this key list.  Such
// a request is strictly ascending and inside the shard's range, because K is,
// so for a Push the check below is the whole validation, and it reads no more
// than the validation pass plus the resolve's store keys would: request key 8
// + store key 8 B / key (k_ident_check).  The apply then streams values only:
// value 4 + store value read/write 8 B / key (k_ident_apply) — 28 B / key for
// the pair, the algorithmic bytes, where validation + resolve-and-apply move
// 36.  A Pull checks its keys on the way: request key 8 + store key 8 + store
// value 4 + reply 4.  Both are plain grid-stride streams, with no per-tile
// state between a lane's loads.
// The host sends a request this way only while the key list's windows are
// trusted and the last identity attempt on it did not fail against this K; a
// request that turns out not to be one writes nothing to the store (Push:
// every block reads kRejIdent first; Pull: only its reply) and reports
// W_NOTIDENT, raising kPending like any follow-up, and the host serves it again
// on the general path.


// The stretch's first slot, uniform: tile 0's cached window is current and is
// for this first key, and n slots fit from it.
__device__ __forceinline__ bool stretch_base(const uint64_t* __restrict__ q, uint64_t n, uint64_t S,
                                             const Win* __restrict__ win, uint32_t gen, uint64_t* D) {
  const Win e = win[0];
  *D = e.lo;
  return e.gen == gen && e.first == q[0] && (uint64_t)e.lo <= S && n <= S - (uint64_t)e.lo;
}

// Push / PushPull, pass 1: q[i] == K[D + i] for every i.  Any failure writes
// seq into rej[kRejIdent] (the apply then writes nothing).
__global__ __launch_bounds__(256) void k_ident_check(const uint64_t* __restrict__ q, uint64_t n,
                                                     const uint64_t* __restrict__ K, uint64_t S,
                                                     const Win* __restrict__ win, uint32_t gen,
                                                     int* __restrict__ rej, int seq, int vec) {
  uint64_t D;
  int bad = 0;
  if (!stretch_base(q, n, S, win, gen, &D)) {
    bad = 1;  // uniform
  } else {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t* Kd = K + D;
    uint64_t done = 0;
    if ((vec & 2) && (D & 1) == 0) {
      // groups of 4 keys (two 16-B loads of each array), kIdU groups per lane
      // in flight, blocks striding over kBlock * kIdU-group tiles
      const uint64_t ng = n / 4;
      done = ng * 4;
      for (uint64_t b = (uint64_t)blockIdx.x * kBlock * kIdU + threadIdx.x; b < ng; b += stride * kIdU) {
        u64x2 a[kIdU][2], c[kIdU][2];
#pragma unroll
        for (int u = 0; u < kIdU; ++u) {
          const uint64_t j = b + (uint64_t)u * kBlock < ng ? b + (uint64_t)u * kBlock : b;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            a[u][h] = *reinterpret_cast<const u64x2*>(q + 4 * j + 2 * h);
            c[u][h] = *reinterpret_cast<const u64x2*>(Kd + 4 * j + 2 * h);
          }
        }
#pragma unroll
        for (int u = 0; u < kIdU; ++u)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            if (a[u][h][0] != c[u][h][0] || a[u][h][1] != c[u][h][1]) bad = 1;
      }
    }
    for (uint64_t i = done + gid; i < n; i += stride)
      if (q[i] != Kd[i]) bad = 1;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) rej[kRejIdent] = seq;
}

// Pass 2 (a Push checked by k_ident_check), or the whole request (a Pull):
// store[D + i] += val[i] and / or out[i] = store[D + i], then the request's
// completion word (block_arrive / request_done, as k_resolve_apply).  A Pull
// whose keys are not the stretch flags W_NOTIDENT (condition bit 2) and its
// reply is rewritten by the general path.
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_ident_apply(const uint64_t* __restrict__ q, uint64_t n,
                                                     const uint64_t* __restrict__ K, uint64_t S,
                                                     const Win* __restrict__ win, uint32_t gen,
                                                     typename Elem<DT>::T* __restrict__ V,
                                                     const typename Elem<DT>::T* __restrict__ vals,
                                                     typename Elem<DT>::T* __restrict__ outv, int* __restrict__ rej,
                                                     int seq, int vec, Arrival arrival, uint32_t* __restrict__ word,
                                                     uint32_t tag_bits) {
  using E = Elem<DT>;
  using T = typename E::T;
  constexpr bool PUSH = (OP & PSG_PUSH) != 0;
  constexpr bool PULL = (OP & PSG_PULL) != 0;
  __shared__ uint32_t s_cond;
  if (threadIdx.x == 0) s_cond = 0;
  __syncthreads();
  uint32_t uniform = rej[kPending] != 0 ? (uint32_t)W_GATED : 0u;
  if constexpr (PUSH) {
    if (rej[kRejIdent] == seq) uniform |= W_NOTIDENT;
  }
  int bad = 0;
  uint64_t D = 0;
  if (!uniform && !stretch_base(q, n, S, win, gen, &D)) {
    // (a Push's check saw the same and rejected it: only a Pull gets here)
    bad = 1;
  } else if (!uniform) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    T* Vd = V + D;
    const uint64_t* Kd = K + D;
    uint64_t done = 0;
    // 16-B vectors of 4-B values: the stretch's first slot 16-B aligned and
    // the caller's arrays too (uniform)
    if (sizeof(T) == 4 && (D & 3) == 0 && (vec & 1) && (PUSH || (vec & 2))) {
      if constexpr (sizeof(T) == 4) {
        const uint64_t ng = n / 4;
        done = ng * 4;
        for (uint64_t b = (uint64_t)blockIdx.x * kBlock * kIdU + threadIdx.x; b < ng; b += stride * kIdU) {
          // kIdU groups of 4 per lane in flight (a lane past the end repeats
          // its first group, unwritten)
          f32x4 x[kIdU], v[kIdU];
          u64x2 a[kIdU][2], c[kIdU][2];
          uint64_t j[kIdU];
#pragma unroll
          for (int u = 0; u < kIdU; ++u) {
            j[u] = b + (uint64_t)u * kBlock < ng ? b + (uint64_t)u * kBlock : b;
            x[u] = __builtin_bit_cast(f32x4, (vec & 8) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Vd + 4 * j[u]))
                                                       : *reinterpret_cast<const u32x4*>(Vd + 4 * j[u]));
            if constexpr (PUSH) {
              v[u] = __builtin_bit_cast(f32x4, (vec & 16) ? reinterpret_cast<const u32x4*>(vals)[j[u]]
                                                        : __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vals) + j[u]));
            } else {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                a[u][h] = *reinterpret_cast<const u64x2*>(q + 4 * j[u] + 2 * h);
                c[u][h] = *reinterpret_cast<const u64x2*>(Kd + 4 * j[u] + 2 * h);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < kIdU; ++u) {
            const bool in = b + (uint64_t)u * kBlock < ng;
            if constexpr (PUSH) {
#pragma unroll
              for (int k = 0; k < 4; ++k) x[u][k] = E::add1(x[u][k], v[u][k]);
              if (in) {
                if (vec & 4)
                  __builtin_nontemporal_store(__builtin_bit_cast(u32x4, x[u]), reinterpret_cast<u32x4*>(Vd + 4 * j[u]));
                else
                  *reinterpret_cast<u32x4*>(Vd + 4 * j[u]) = __builtin_bit_cast(u32x4, x[u]);
              }
            } else {
#pragma unroll
              for (int h = 0; h < 2; ++h)
                if (a[u][h][0] != c[u][h][0] || a[u][h][1] != c[u][h][1]) bad = 1;
            }
            if constexpr (PULL)
              if (in)
                __builtin_nontemporal_store(__builtin_bit_cast(u32x4, x[u]), reinterpret_cast<u32x4*>(outv) + j[u]);
          }
        }
      }
    }
    for (uint64_t i = done + gid; i < n; i += stride) {
      T x = Vd[i];
      if constexpr (PUSH) {
        x = E::add1(x, vals[i]);
        Vd[i] = x;
      } else {
        if (q[i] != Kd[i]) bad = 1;
      }
      if constexpr (PULL) outv[i] = x;
    }
  }
  const uint64_t after = block_arrive(bad ? 2u : 0u, &s_cond, arrival);
  request_done(after, arrival, uniform, rej + kPending, word, tag_bits, W_NOTIDENT);
}

// A slot list that is a stretch of the store: slots[i] == slots[0] + i for
// every i (psg_store_slots_stretch).  Any other list raises F_MISSING (here:
// "not a stretch").
__global__ __launch_bounds__(256) void k_slots_stretch(const uint32_t* __restrict__ slots, uint64_t n,
                                                       int* __restrict__ flags) {
  const uint64_t s0 = slots[0];
  int bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    if ((uint64_t)slots[i] != s0 + i) bad = 1;
  raise_flag(flags, F_MISSING, bad != 0);
}

// Merge: old element j goes to j + #(new keys < K[j]); new key t goes to
// t + #(old keys < M[t]).
template <typename T>
__global__ __launch_bounds__(256) void k_merge_old(const uint64_t* __restrict__ K,
                                                   const T* __restrict__ V, uint64_t S,
                                                   const uint64_t* __restrict__ M, uint64_t m,
                                                   uint64_t* __restrict__ K2, T* __restrict__ V2) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < S;
       j += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = K[j];
    const uint64_t d = j + lower_bound_dev(M, 0, m, key);
    K2[d] = key;
    V2[d] = V[j];
  }
}
template <typename T>
__global__ __launch_bounds__(256) void k_merge_new(const uint64_t* __restrict__ K, uint64_t S,
                                                   const uint64_t* __restrict__ M, uint64_t m,
                                                   uint64_t* __restrict__ K2, T* __restrict__ V2) {
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < m;
       t += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = M[t];
    const uint64_t d = t + lower_bound_dev(K, 0, S, key);
    K2[d] = key;
    V2[d] = (T)0.0f;
  }
}

// DENSE store addressed by explicit keys: slot = key - key_begin.
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_dense_keyed(typename Elem<DT>::T* __restrict__ store,
                                                     uint64_t kb, uint64_t cap,
                                                     const uint64_t* __restrict__ keys,
                                                     const typename Elem<DT>::T* __restrict__ vals,
                                                     typename Elem<DT>::T* __restrict__ out,
                                                     uint64_t n, const int* __restrict__ reject,
                                                     int seq) {
  using E = Elem<DT>;
  if (reject[kRejRange] == seq || reject[kRejUnsorted] == seq) return;  // rejected by k_validate_keys
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t p = keys[i] - kb;
    typename E::T s = store[p];
    if constexpr ((OP & PSG_PUSH) != 0) {
      s = E::add1(s, vals[i]);
      store[p] = s;
    }
    if constexpr ((OP & PSG_PULL) != 0) out[i] = s;
  }
}

// Slots of a DENSE store: key - key_begin (kNoSlot when outside).
__global__ __launch_bounds__(256) void k_dense_slots(const uint64_t* __restrict__ keys, uint64_t n,
                                                     uint64_t kb, uint64_t cap,
                                                     uint32_t* __restrict__ slots,
                                                     int* __restrict__ flags) {
  int bad = 0, unsorted = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = keys[i];
    if (i > 0 && keys[i - 1] >= key) unsorted = 1;
    const uint64_t p = key - kb;
    const bool ok = key >= kb && p < cap && p < 0xffffffffull;
    if (!ok) bad = 1;
    slots[i] = ok ? (uint32_t)p : kNoSlot;
  }
  raise_flag(flags, F_RANGE, bad != 0);
  raise_flag(flags, F_UNSORTED, unsorted != 0);
}

// zero the request flags (host memory) before a flag-raising launch; the
// previous request on this store has synchronised its stream
static void reset_flags(psg_store* s) { memset(s->flags_host, 0, F_NFLAGS * sizeof(int)); }

static unsigned grid_n(uint64_t n, uint64_t per_block) {
  uint64_t b = (n + per_block - 1) / per_block;
  uint64_t cap = (uint64_t)max_stream_blocks();
  if (b > cap) b = cap;
  return b ? (unsigned)b : 1u;
}

static int ensure_slots(psg_store* s, uint64_t n) {
  if (s->slots_cap >= n) return PSG_OK;
  if (s->slots) PSG_HIP(hipFree(s->slots));
  if (s->slots2) PSG_HIP(hipFree(s->slots2));
  if (s->wlo) PSG_HIP(hipFree(s->wlo));
  s->slots = s->slots2 = nullptr;
  s->wlo = nullptr;
  s->slots_cap = 0;
  uint64_t cap = std::max<uint64_t>(n, 1 << 16);
  PSG_HIP(hipMalloc(&s->slots, cap * sizeof(uint32_t)));
  PSG_HIP(hipMalloc(&s->slots2, cap * sizeof(uint32_t)));
  PSG_HIP(hipMalloc(&s->wlo, (cap / kTile + 2) * sizeof(uint64_t)));
  s->slots_cap = cap;
  return PSG_OK;
}

// Launch the two resolve passes for q into `slots` (no host sync).
static int launch_resolve(psg_store* s, const uint64_t* q, uint64_t n, uint32_t* slots,
                          hipStream_t st) {
  const uint64_t ntiles = (n + kTile - 1) / kTile;
  reset_flags(s);
  k_tile_windows<<<grid_n(ntiles + 1, kBlock / 64), kBlock, 0, st>>>(q, n, s->keys, s->size, s->wlo, kTile);
  k_resolve<<<grid_n(ntiles, 1), kBlock, 0, st>>>(q, n, s->keys, s->size, s->wlo, s->key_begin,
                                                  s->key_end, slots, s->flags);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

static int check_request_flags(psg_store* s) {
  const int* f = s->flags_host;
  PSG_REQUIRE(!f[F_UNSORTED], PSG_ERR_INVALID,
              "request keys are not strictly ascending (KVPairs contract, KVApp.h:23)");
  PSG_REQUIRE(!f[F_RANGE], PSG_ERR_RANGE, "request key outside the store range [%llu, %llu)",
              (unsigned long long)s->key_begin, (unsigned long long)s->key_end);
  return PSG_OK;
}

// Apply the request to the keys that were absent in the first pass
// (old[i] == kNoSlot), now inserted at new[i].
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_slots_fixup(typename Elem<DT>::T* __restrict__ store,
                                                     const uint32_t* __restrict__ old_slots,
                                                     const uint32_t* __restrict__ new_slots,
                                                     const typename Elem<DT>::T* __restrict__ vals,
                                                     typename Elem<DT>::T* __restrict__ out,
                                                     uint64_t n) {
  using E = Elem<DT>;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    if (old_slots[i] != kNoSlot) continue;
    const uint32_t p = new_slots[i];
    typename E::T v = store[p];
    if constexpr ((OP & PSG_PUSH) != 0) {
      v = E::add1(v, vals[i]);
      store[p] = v;
    }
    if constexpr ((OP & PSG_PULL) != 0) out[i] = v;
  }
}

template <int DT>
static int run_fixup(psg_store* s, int op, const void* vals, void* out, uint64_t n, hipStream_t st) {
  using T = typename Elem<DT>::T;
  const unsigned g = grid_n(n, kBlock);
  T* sv = (T*)s->vals;
  switch (op) {
    case PSG_PUSH:
      k_slots_fixup<DT, PSG_PUSH><<<g, kBlock, 0, st>>>(sv, s->slots, s->slots2, (const T*)vals, (T*)out, n);
      break;
    case PSG_PULL:
      k_slots_fixup<DT, PSG_PULL><<<g, kBlock, 0, st>>>(sv, s->slots, s->slots2, (const T*)vals, (T*)out, n);
      break;
    default:
      k_slots_fixup<DT, PSG_PUSH | PSG_PULL><<<g, kBlock, 0, st>>>(sv, s->slots, s->slots2,
                                                                  (const T*)vals, (T*)out, n);
  }
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// Wait for everything enqueued on a stream so far, with its writes visible to
// the host, to copies and to other agents, without sleeping in the runtime:
// an event recorded behind the work, polled with hipEventQuery — the runtime's
// own completion test, which promises what hipEventSynchronize promises — and
// hipEventSynchronize after 2 ms (a long request, or a fault: it also reports
// the error).  PSG_SYNC_POLL=0 always takes hipStreamSynchronize (A/B).
//
// Round 3 polled a word the stream wrote into pinned memory instead
// (hipStreamWriteValue32), whose documentation promises only that the write
// follows the earlier commands' execution, nothing about their writes being
// visible to the next reader.  Every hand-off now rests on the documented
// event semantics: a hardening step.  (GPUTEST_r03's red LR case was not a
// hand-off: the reference LRServer installs its handle before InitWeight
// runs, LRServer.h:70 vs 81-87 — DESIGN.md, "Parity".)
static bool sync_poll() {
  static const bool on = [] {
    const char* e = getenv("PSG_SYNC_POLL");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

static int poll_event(hipEvent_t ev) {
  auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; ++spin) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return PSG_OK;
    if (q != hipErrorNotReady) return hip_fail(q, "hipEventQuery", __FILE__, __LINE__);
    if ((spin & 15) == 15 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    __builtin_ia32_pause();
  }
  PSG_HIP(hipEventSynchronize(ev));
  return PSG_OK;
}

static int stream_done(psg_store* s, hipStream_t st) {
  if (sync_poll() && s->done_ev) {
    PSG_HIP(hipEventRecord(s->done_ev, st));
    return poll_event(s->done_ev);
  }
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

// The request's kernels done; then the host may read flags_host (the kernels
// wrote it directly, system-scope stores into pinned memory).
static int read_flags(psg_store* s, hipStream_t st) { return stream_done(s, st); }

template <typename T>
static int merge_insert(psg_store* s, const uint64_t* miss, uint64_t m, hipStream_t st) {
  const uint64_t S = s->size;
  uint64_t cap = s->capacity;
  if (S + m > cap) {
    cap = std::max<uint64_t>(S + m, cap * 2);
    cap = std::max<uint64_t>(cap, 1024);
  }
  PSG_REQUIRE(cap <= 0xfffffffeull, PSG_ERR_RANGE, "SORTED store: more than 2^32-2 keys");
  uint64_t* K2 = nullptr;
  T* V2 = nullptr;
  PSG_HIP(hipMalloc((void**)&K2, (cap + kKeyPad) * sizeof(uint64_t)));
  // whole 2 MiB pages: the value array is what peers map for the keyed xGMI
  // exchange (psg_xgmi_push_slots / _pull_slots)
  PSG_HIP(hipMalloc((void**)&V2, ipc_alloc_bytes(cap * sizeof(T))));
  if (S) k_merge_old<T><<<grid_n(S, kBlock), kBlock, 0, st>>>(s->keys, (const T*)s->vals, S, miss, m, K2, V2);
  k_merge_new<T><<<grid_n(m, kBlock), kBlock, 0, st>>>(s->keys, S, miss, m, K2, V2);
  PSG_HIP(hipGetLastError());
  PSG_HIP(hipStreamSynchronize(st));
  if (s->keys) PSG_HIP(hipFree(s->keys));
  if (s->vals) PSG_HIP(hipFree(s->vals));
  s->keys = K2;
  s->vals = V2;
  s->size = S + m;
  s->capacity = cap;
  s->gen++;  // every cached window belongs to the old K
  return PSG_OK;
}

static int insert_missing(psg_store* s, const uint64_t* q, uint64_t n, hipStream_t st) {
  const uint64_t ntiles = compact_tiles(n);
  const SlotIs absent = {s->slots, kNoSlot};
  uint32_t* counts = nullptr;
  uint64_t* miss = nullptr;
  PSG_HIP(hipMalloc((void**)&counts, (ntiles + 1) * sizeof(uint32_t)));
  compact_count(n, counts, absent, st);
  uint64_t m = 0;
  PSG_TRY(read_count(counts + ntiles, &m, st));
  if (m == 0) {
    PSG_HIP(hipFree(counts));
    return PSG_OK;
  }
  PSG_HIP(hipMalloc((void**)&miss, m * sizeof(uint64_t)));
  compact_emit(n, counts, absent, EmitKey{q, miss}, st);
  PSG_HIP(hipGetLastError());
  int rc;
  switch (s->dtype) {
    case PSG_F32: rc = merge_insert<float>(s, miss, m, st); break;
    case PSG_F64: rc = merge_insert<double>(s, miss, m, st); break;
    case PSG_F16: rc = merge_insert<_Float16>(s, miss, m, st); break;
    case PSG_BF16: rc = merge_insert<__bf16>(s, miss, m, st); break;
    default: rc = PSG_ERR_UNSUPPORTED;
  }
  PSG_HIP(hipStreamSynchronize(st));
  PSG_HIP(hipFree(counts));
  PSG_HIP(hipFree(miss));
  return rc;
}

// One request on the SORTED store with ONE host synchronisation in the steady
// state: resolve (2 kernels) -> gather/scatter over the slots (absent keys
// skipped; a pull of an absent key reads 0, which is what its insertion
// gives) -> read the flags.  Only when keys were absent: insert them (merge),
// resolve again into slots2, and apply the request to exactly those keys.
// Block size of the fused kernel (PSG_RA_BLOCK = 256 | 512 | 1024, default
// 1024).  The tile is 4 keys per lane, so a larger block leaves fewer windows
// to search (10 M keys: k_tile_windows 11.2 -> 8.8 us from 256 to 512; keyed
// Push+Pull 606 / 660 / 675 GB/s at 256 / 512 / 1024).
// A request sparse in the store (the store holds more than twice as many
// keys as the request asks for — an LR minibatch) gets 256-thread blocks
// instead: its tiles' windows span more store keys than they have keys, and
// smaller windows let 8 blocks per CU stage theirs at once instead of 2
// (round 4, on the general path: every 2nd key of a 20 M-key store, keyed
// Push+Pull 484 against 455-459 GB/s, profiles/r4_ab_ra_block_sparse.txt;
// since round 6 a request of at least every other store key keeps 1024, below).
static int ra_block(const psg_store* s, uint64_t n) {
  static const int env = [] {
    const char* e = getenv("PSG_RA_BLOCK");
    const int v = e ? atoi(e) : 0;
    return v == 256 || v == 512 || v == 1024 ? v : 0;
  }();
  if (env) return env;
  // at least every other store key: 1024-thread tiles, whose windows (at most
  // 8192 store keys for 4096 request keys) take coded tiles, the lean apply
  // and the verified copy — every other key of a 20 M-key store, Push 0.38 ->
  // 0.51 of HBM, Push+Pull 510 -> 585 GB/s against 256-thread tiles (the Pull
  // alone 0.45 -> 0.43; profiles/r6_keyed_sparse_block_ab.txt)
  return s->size > 2 * n ? 256 : 1024;
}

// The window cache entry for request keys (q, n): the entry last filled for
// them, else the least recently used one (its windows stay correct for any
// tile whose end keys they match, so it needs no clearing).
static psg_store::WinCache* win_entry(psg_store* s, const uint64_t* q, uint64_t n, uint64_t ntiles,
                                      hipStream_t st) {
  psg_store::WinCache* e = nullptr;
  for (auto& c : s->wc)
    if (c.win && c.q == q && c.n == n) e = &c;
  if (!e) {
    e = &s->wc[0];
    for (auto& c : s->wc)
      if (c.last_use < e->last_use) e = &c;
    e->q = q;
    e->n = n;
    e->trusted = 0;
    e->strikes = 0;
    e->ident_fail = 0;
    e->lean_fail = 0;
    e->ident_ok = 0;
    e->ident_trial = 0;
    e->copy_gen = 0;
    e->vl_fail = 0;
    e->learn_ticket = 0;
  }
  if (e->cap_tiles < ntiles) {
    if (e->win) (void)hipFree(e->win);
    if (e->codes) (void)hipFree(e->codes);
    if (e->copy) (void)hipFree(e->copy);
    e->win = nullptr;
    e->codes = nullptr;
    e->copy = nullptr;
    e->copy_cap = 0;
    e->copy_gen = 0;
    e->cap_tiles = 0;
    const uint64_t cap = std::max<uint64_t>(ntiles, 64);
    if (hipMalloc(&e->win, cap * sizeof(Win)) != hipSuccess) return nullptr;
    // (the lane codes of its coded tiles, 1 B per key, are allocated with
    // the first Push that validates them: launch_fused)
    // gen 0 never matches a store generation: a fresh entry is all misses
    // (stream-ordered before the request's kernels, which fill it)
    if (hipMemsetAsync(e->win, 0, cap * sizeof(Win), st) != hipSuccess) return nullptr;
    e->cap_tiles = cap;
    e->trusted = 0;
    // the stretch-tile words (k_validate_windows chunk_ok) hold one per tile of
    // the largest entry; grown here, where the requests in flight have been
    // drained (launch_fused), seq never 0 so zeroed words mark nothing
    if (s->chunk_cap < cap) {
      if (s->chunk_ok) (void)hipFree(s->chunk_ok);
      s->chunk_ok = nullptr;
      s->chunk_cap = 0;
      // one set per ring slot: a request's tile words stay its own while later
      // requests in flight validate theirs (a follow-up of k_tile_apply reads
      // them after those ran)
      if (hipMalloc(&s->chunk_ok, (uint64_t)kRing * cap * sizeof(int)) != hipSuccess) return nullptr;
      if (hipMemsetAsync(s->chunk_ok, 0, (uint64_t)kRing * cap * sizeof(int), st) != hipSuccess) return nullptr;
      s->chunk_cap = cap;
    }
  }
  e->last_use = ++s->wc_clock;
  return e;
}

// ---- the out-of-order path ------------------------------------------------
// KVServerDefaultHandle walks a request in arrival order (KVApp.h:446-454):
// `store[key] += vals[i]` per occurrence, and a PushPull answers the running
// value.  A request whose keys are not strictly ascending — any order, keys
// repeated — is therefore served by resolving every key (any order), inserting
// the absent ones, sorting the (slot, position) pairs by slot STABLY (each
// key's occurrences stay in arrival order; psg_sort.hip), and walking each
// slot's run in order: one lane per run adds its occurrences one after the
// other, exactly the reference's sequence of additions, and writes each
// occurrence's running value to its reply position.

// slots[i] = index of q[i] in K[0..S), or kNoSlot (any order, repeats allowed)
__global__ __launch_bounds__(256) void k_resolve_any(const uint64_t* __restrict__ q, uint64_t n,
                                                     const uint64_t* __restrict__ K, uint64_t S,
                                                     uint32_t* __restrict__ slots) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = q[i];
    const uint64_t p = lower_bound_dev(K, 0, S, key);
    slots[i] = (p < S && K[p] == key) ? (uint32_t)p : kNoSlot;
  }
}

// One lane per run of equal slots in the slot-sorted pairs (ss, sp): the
// occurrences in arrival order, each added in turn (Push), each reply the
// running value (PushPull).
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_seg_apply(const uint32_t* __restrict__ ss, const uint32_t* __restrict__ sp,
                                                   uint64_t n, typename Elem<DT>::T* __restrict__ V,
                                                   const typename Elem<DT>::T* __restrict__ vals,
                                                   typename Elem<DT>::T* __restrict__ out) {
  using E = Elem<DT>;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t slot = ss[j];
    if (j > 0 && ss[j - 1] == slot) continue;  // not the head of its run
    typename E::T acc = V[slot];
    uint64_t k = j;
    do {
      const uint32_t p = sp[k];
      acc = E::add1(acc, vals[p]);
      if constexpr ((OP & PSG_PULL) != 0) out[p] = acc;
      ++k;
    } while (k < n && ss[k] == slot);
    V[slot] = acc;
  }
}

// Scratch of the out-of-order path, carved from one growing device block.
struct GScratch {
  uint32_t *a, *b, *c, *counts, *tcount;
  uint64_t *k0, *k1;
};
static int general_scratch(psg_store* s, uint64_t n, GScratch* g) {
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  const uint64_t nt = compact_tiles(n) + 2;
  const uint64_t u32n = al(n * 4), u64n = al(n * 8), cnt = al(radix_counts_elems(n) * 4), tc = al(nt * 4);
  const uint64_t bytes = 3 * u32n + cnt + tc + 2 * u64n;
  if (s->gbuf_bytes < bytes) {
    if (s->gbuf) PSG_HIP(hipFree(s->gbuf));
    s->gbuf = nullptr;
    s->gbuf_bytes = 0;
    PSG_HIP(hipMalloc(&s->gbuf, bytes));
    s->gbuf_bytes = bytes;
  }
  char* p = (char*)s->gbuf;
  g->a = (uint32_t*)p, p += u32n;
  g->b = (uint32_t*)p, p += u32n;
  g->c = (uint32_t*)p, p += u32n;
  g->counts = (uint32_t*)p, p += cnt;
  g->tcount = (uint32_t*)p, p += tc;
  g->k0 = (uint64_t*)p, p += u64n;
  g->k1 = (uint64_t*)p;
  return PSG_OK;
}

// The absent keys of q[0..n) (s->slots[i] == kNoSlot; any order, repeats)
// inserted with value 0 (operator[], KVApp.h:449/452): compacted, sorted,
// made unique, merged into K.  *inserted = how many.
static int insert_missing_any(psg_store* s, const uint64_t* q, uint64_t n, const GScratch& g, uint64_t* inserted,
                              hipStream_t st) {
  *inserted = 0;
  const SlotIs absent = {s->slots, kNoSlot};
  compact_count(n, g.tcount, absent, st);
  uint64_t m = 0;
  PSG_TRY(read_count(g.tcount + compact_tiles(n), &m, st));
  if (m == 0) return PSG_OK;
  compact_emit(n, g.tcount, absent, EmitKey{q, g.k0}, st);
  int res = 0;
  PSG_TRY(radix_sort_u64(g.k0, g.a, m, 64, true, g.k1, g.b, g.counts, st, &res));
  const uint64_t* sorted = res ? g.k1 : g.k0;
  uint64_t* uniq = res ? g.k0 : g.k1;
  compact_count(m, g.tcount, RunHead{sorted}, st);
  uint64_t mu = 0;
  PSG_TRY(read_count(g.tcount + compact_tiles(m), &mu, st));
  compact_emit(m, g.tcount, RunHead{sorted}, EmitKey{sorted, uniq}, st);
  PSG_HIP(hipGetLastError());
  switch (s->dtype) {
    case PSG_F32: PSG_TRY(merge_insert<float>(s, uniq, mu, st)); break;
    case PSG_F64: PSG_TRY(merge_insert<double>(s, uniq, mu, st)); break;
    case PSG_F16: PSG_TRY(merge_insert<_Float16>(s, uniq, mu, st)); break;
    case PSG_BF16: PSG_TRY(merge_insert<__bf16>(s, uniq, mu, st)); break;
    default: return PSG_ERR_UNSUPPORTED;
  }
  *inserted = mu;
  return PSG_OK;
}

static int bit_width(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; }

// A request whose keys are not strictly ascending (already checked to lie in
// the store's range), served in arrival order.  Synchronous.
template <int DT>
static int general_request(psg_store* s, int op, const uint64_t* q, const void* vals, void* out, uint64_t n,
                           hipStream_t st) {
  using T = typename Elem<DT>::T;
  s->counters[PSG_CTR_ORDERED]++;
  PSG_TRY(ensure_slots(s, n));
  GScratch g;
  PSG_TRY(general_scratch(s, n, &g));
  uint32_t* slots = s->slots;
  uint64_t slot_space;
  if (s->kind == PSG_STORE_SORTED) {
    if (s->size) k_resolve_any<<<grid_n(n, kBlock), kBlock, 0, st>>>(q, n, s->keys, s->size, slots);
    else PSG_HIP(hipMemsetAsync(slots, 0xff, n * sizeof(uint32_t), st));
    uint64_t inserted = 0;
    PSG_TRY(insert_missing_any(s, q, n, g, &inserted, st));
    if (inserted) k_resolve_any<<<grid_n(n, kBlock), kBlock, 0, st>>>(q, n, s->keys, s->size, slots);
    slot_space = s->size;
  } else {
    reset_flags(s);
    k_dense_slots<<<grid_n(n, kBlock), kBlock, 0, st>>>(q, n, s->key_begin, s->capacity, slots, s->flags);
    slot_space = s->capacity;
  }
  PSG_HIP(hipGetLastError());
  if (op == PSG_PULL) {  // reads only: every occurrence gets its key's value
    PSG_TRY(slot_request(s->dtype, PSG_PULL, s->vals, slots, nullptr, out, n, st));
  } else {
    int res = 0;
    const int bits = std::max(1, bit_width(slot_space ? slot_space - 1 : 0));
    PSG_TRY(radix_sort_u32(slots, g.a, n, bits, true, g.b, g.c, g.counts, st, &res));
    const uint32_t* ss = res ? g.b : slots;
    const uint32_t* sp = res ? g.c : g.a;
    const unsigned gr = grid_n(n, kBlock);
    if (op == PSG_PUSH)
      k_seg_apply<DT, PSG_PUSH><<<gr, kBlock, 0, st>>>(ss, sp, n, (T*)s->vals, (const T*)vals, (T*)out);
    else
      k_seg_apply<DT, PSG_PUSH | PSG_PULL><<<gr, kBlock, 0, st>>>(ss, sp, n, (T*)s->vals, (const T*)vals, (T*)out);
    PSG_HIP(hipGetLastError());
  }
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

static int general_dispatch(psg_store* s, int op, const uint64_t* q, const void* vals, void* out, uint64_t n,
                            hipStream_t st) {
  switch (s->dtype) {
    case PSG_F32: return general_request<PSG_F32>(s, op, q, vals, out, n, st);
    case PSG_F64: return general_request<PSG_F64>(s, op, q, vals, out, n, st);
    case PSG_F16: return general_request<PSG_F16>(s, op, q, vals, out, n, st);
    default: return general_request<PSG_BF16>(s, op, q, vals, out, n, st);
  }
}

// ---- fused requests, in flight -------------------------------------------
// A new request: its sequence number tags the reject words (never reset: a
// stale value names an older request).
static int next_seq(psg_store* s) {
  s->seq = s->seq == 0x7fffffff ? 1 : s->seq + 1;
  return s->seq;
}
static uint32_t next_tag(psg_store* s) {
  s->tag = (s->tag + 1) & 0xffffffu;
  if (s->tag == 0) s->tag = 1;
  return s->tag;
}

static int drain(psg_store* s);

// The tile words of the request validated in ring slot `ring`.
static uint32_t* tile_words(psg_store* s, uint32_t ring) {
  return reinterpret_cast<uint32_t*>(s->chunk_ok) + (uint64_t)ring * s->chunk_cap;
}


// Launch one fused request — k_validate_windows (skipped for a Pull on
// trusted windows), then k_resolve_apply — and return without waiting.  Its
// completion word arrives in ring slot rec->ring.
template <int DT, int OP>
static void launch_apply(psg_store* s, const uint64_t* q, uint64_t n, const void* vals, void* out, Win* win,
                         const InflightReq& rec, hipStream_t st) {
  using T = typename Elem<DT>::T;
  const int nt = rec.nt;
  const uint64_t ntiles = (n + (uint64_t)nt * kPerLane - 1) / ((uint64_t)nt * kPerLane);
  // bit 0: request values / replies 16-B aligned; bit 1: request keys 16-B aligned
  // a Push sparse in its store (256-thread tiles) writes whole 8-slot spans
  // where it may (k_resolve_apply<.., SP>): every 2nd key of a 20 M-key store,
  // Push 112-113 -> 102 us, Push+Pull 488-490 -> 508-510 GB/s; a standalone
  // probe of that store traffic, 3.5 -> 5.6 TB/s (partly written lines cost
  // the memory a read-modify-write of their own; profiles/r4_ab_sparse_span.txt).
  // PSG_RA_VECW=0: never (A/B)
  static const int vecw = [] {
    const char* e = getenv("PSG_RA_VECW");
    return e ? atoi(e) : 1;
  }();
  const int vec = (((OP & PSG_PUSH) == 0 || aligned16(vals)) && ((OP & PSG_PULL) == 0 || aligned16(out)) ? 1 : 0) |
                  (aligned16(q) ? 2 : 0) | (vecw && aligned16(s->vals) ? 4 : 0) | (rec.lean == 2 ? 8 : 0);
  const unsigned g = grid_n(ntiles, 1);
  Arrival arr;
  arr.ctr = s->done_ctr + (uint64_t)rec.ring * (kArriveShards + 1) * kArriveStride;
#define PSG_RA_ARGS                                                                                     \
  q, n, s->keys, s->size, win, s->gen, s->key_begin, s->key_end, (T*)s->vals, (const T*)vals, (T*)out, \
      s->reject_dev, rec.seq, vec, arr, s->ring_dev + rec.ring, rec.tag << 8,                           \
      rec.mident ? tile_words(s, rec.tw_ring) : nullptr, s->wc[rec.wc].codes
  // the 256-thread tiles of a request at most 2 in 5 of whose store's keys it
  // asks for stage windows of 4 tiles (32 KiB: 4 blocks per CU instead of 8)
  // — every 3rd key of the store: Push+Pull 333 -> 361 GB/s, every 4th 266 ->
  // 276; every 2nd keeps 2 tiles (512 against 465 with 4;
  // profiles/r4_ab_sparse_window.txt)
  const bool wide = nt == 256 && 2 * s->size >= 5 * n;
  if (nt == 1024 && rec.mident && (OP & PSG_PUSH))
    k_resolve_apply<DT, OP, 1024, false, 2, true><<<g, 1024, 0, st>>>(PSG_RA_ARGS);
  else if (nt == 1024)
    k_resolve_apply<DT, OP, 1024><<<g, 1024, 0, st>>>(PSG_RA_ARGS);
  else if (nt == 256 && (vec & 4) && (OP & PSG_PUSH) && sizeof(T) == 4 && wide)
    k_resolve_apply<DT, OP, 256, true, 4><<<g, 256, 0, st>>>(PSG_RA_ARGS);
  else if (nt == 256 && (vec & 4) && (OP & PSG_PUSH) && sizeof(T) == 4)
    k_resolve_apply<DT, OP, 256, true><<<g, 256, 0, st>>>(PSG_RA_ARGS);
  else if (nt == 256 && wide)
    k_resolve_apply<DT, OP, 256, false, 4><<<g, 256, 0, st>>>(PSG_RA_ARGS);
  else if (nt == 512)
    k_resolve_apply<DT, OP, 512><<<g, 512, 0, st>>>(PSG_RA_ARGS);
  else
    k_resolve_apply<DT, OP, 256><<<g, 256, 0, st>>>(PSG_RA_ARGS);
#undef PSG_RA_ARGS
}

// Launch k_tile_apply for a Push whose coded validation has run (launch_fused).
template <int DT, int OP>
static void launch_tile_apply(psg_store* s, uint64_t n, const void* vals, void* out, Win* win,
                              const InflightReq& rec, hipStream_t st) {
  using T = typename Elem<DT>::T;
  if constexpr (sizeof(T) == 4) {
    const uint64_t ntiles = (n + 4095) / 4096;
    const unsigned cus = (unsigned)(max_stream_blocks() / 8);
    // PSG_TA_BPC (A/B): blocks per CU in the grid (0: one block per tile)
    static const int ta_bpc = [] {
      const char* e = getenv("PSG_TA_BPC");
      return e ? atoi(e) : 2;
    }();
    const unsigned g = (unsigned)(ta_bpc > 0 ? std::min<uint64_t>(ntiles, (uint64_t)cus * ta_bpc) : ntiles);
    // PSG_TA_NT=0 (A/B): the request's values read as plain loads (vec bit 4)
    static const int ta_nt = [] {
      const char* e = getenv("PSG_TA_NT");
      return e ? atoi(e) : 1;
    }();
    const int vec = (((OP & PSG_PUSH) == 0 || aligned16(vals)) && ((OP & PSG_PULL) == 0 || aligned16(out)) ? 1 : 0) |
                    (ta_nt ? 0 : 16);
    Arrival arr;
    arr.ctr = s->done_ctr + (uint64_t)rec.ring * (kArriveShards + 1) * kArriveStride;
    static const bool db = [] {
      const char* e = getenv("PSG_TA_DB");
      return e ? atoi(e) != 0 : true;
    }();
    if (db)
      k_tile_apply_db<DT, OP><<<g, 1024, 0, st>>>(n, win, (T*)s->vals, (const T*)vals, (T*)out, s->reject_dev,
                                                  rec.seq, vec, arr, s->ring_dev + rec.ring, rec.tag << 8,
                                                  tile_words(s, rec.tw_ring), s->wc[rec.wc].codes);
    else
      k_tile_apply<DT, OP><<<g, 1024, 0, st>>>(n, win, (T*)s->vals, (const T*)vals, (T*)out, s->reject_dev, rec.seq,
                                               vec, arr, s->ring_dev + rec.ring, rec.tag << 8,
                                               tile_words(s, rec.tw_ring), s->wc[rec.wc].codes);
  }
}

// PSG_RA_IDENT=0: never the identity kernels (A/B)
static bool ident_on() {
  static const bool on = [] {
    const char* e = getenv("PSG_RA_IDENT");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

// Launch one identity request: k_ident_check (Push, PushPull), then
// k_ident_apply, which writes the request's completion word.
template <int DT, int OP>
static void launch_ident(psg_store* s, const uint64_t* q, uint64_t n, const void* vals, void* out, const Win* win,
                         const InflightReq& rec, hipStream_t st) {
  using T = typename Elem<DT>::T;
  // PSG_ID_BPC / PSG_ID_CHECK_BPC (A/B): blocks of 256 per CU of the apply / the
  // check (default 8, the streaming grid)
  static const int id_bpc = [] {
    const char* e = getenv("PSG_ID_BPC");
    const int v = e ? atoi(e) : 0;
    return v >= 1 && v <= 16 ? v : 8;
  }();
  static const int idc_bpc = [] {
    const char* e = getenv("PSG_ID_CHECK_BPC");
    const int v = e ? atoi(e) : 0;
    return v >= 1 && v <= 16 ? v : 8;
  }();
  const unsigned g0 = grid_n(n, (uint64_t)kBlock * 4 * kIdU);
  const unsigned cus = (unsigned)(max_stream_blocks() / 8);
  const unsigned g = std::min<unsigned>(g0, cus * (unsigned)id_bpc);
  const unsigned gc = std::min<unsigned>(g0, cus * (unsigned)idc_bpc);
  // PSG_ID_NT (A/B): bit 0 the store values written non-temporally, bit 1 read so,
  // bit 2 the request's values read as plain loads
  static const int id_nt = [] {
    const char* e = getenv("PSG_ID_NT");
    return e ? atoi(e) : 0;
  }();
  const int vec = (((OP & PSG_PUSH) == 0 || aligned16(vals)) && ((OP & PSG_PULL) == 0 || aligned16(out)) ? 1 : 0) |
                  (aligned16(q) ? 2 : 0) | ((id_nt & 1) ? 4 : 0) | ((id_nt & 2) ? 8 : 0) |
                  ((id_nt & 4) ? 16 : 0);
  if (OP & PSG_PUSH)
    k_ident_check<<<gc, kBlock, 0, st>>>(q, n, s->keys, s->size, win, s->gen, s->reject_dev, s->seq, vec);
  Arrival arr;
  arr.ctr = s->done_ctr + (uint64_t)rec.ring * (kArriveShards + 1) * kArriveStride;
  k_ident_apply<DT, OP><<<g, kBlock, 0, st>>>(q, n, s->keys, s->size, win, s->gen, (T*)s->vals, (const T*)vals,
                                                (T*)out, s->reject_dev, s->seq, vec, arr, s->ring_dev + rec.ring,
                                                rec.tag << 8);
}

template <int DT>
static int launch_fused(psg_store* s, int op, const uint64_t* q, uint64_t n, const void* vals, void* out,
                        hipStream_t st, InflightReq* rec, bool want_land) {
  const int nt = ra_block(s, n);
  const uint64_t tile = (uint64_t)nt * kPerLane;
  const uint64_t ntiles = (n + tile - 1) / tile;
  // the window-cache entry (win_entry's choice): requests in flight may share
  // one — every kernel checks each window against its own tile's end keys and
  // K's generation — but growing one frees windows an in-flight kernel may
  // still read, so that waits for them first
  if (!s->inflight.empty()) {
    const psg_store::WinCache* pick = nullptr;
    for (auto& c : s->wc)
      if (c.win && c.q == q && c.n == n) pick = &c;
    if (!pick) {
      pick = &s->wc[0];
      for (auto& c : s->wc)
        if (c.last_use < pick->last_use) pick = &c;
    }
    if (pick->cap_tiles < ntiles) PSG_TRY(drain(s));
  }
  psg_store::WinCache* wc = win_entry(s, q, n, ntiles, st);
  PSG_REQUIRE(wc, PSG_ERR_HIP, "SORTED store: window cache allocation failed");
  if (wc->nt != nt) {
    // windows filled for another tile size (the store grew past the sparse
    // threshold): searched again, and no verdict carried over
    wc->nt = nt;
    wc->trusted = 0;
    wc->strikes = 0;
    wc->ident_fail = 0;
    wc->lean_fail = 0;
    wc->ident_ok = 0;
  }
  Win* win = static_cast<Win*>(wc->win);
  static const int cache_on = [] {
    const char* e = getenv("PSG_WIN_CACHE");  // 0: always run the search pre-pass (A/B)
    return e ? atoi(e) : 1;
  }();
  const bool trusted = cache_on && wc->trusted != 0 && (uint32_t)wc->trusted == s->gen;
  // trusted windows of a key list whose identity attempt has not failed
  // against this K: the identity kernels (no validation pass, no search)
  // ... and one speculative attempt at a time: until an identity request on
  // this list has completed as one against this K, the requests launched
  // behind an attempt in flight take the general path (a list that is not a
  // stretch would otherwise have every request in flight attempted, rejected
  // and replayed before the first verdict is reaped)
  bool ident = trusted && ident_on() && wc->ident_fail != s->gen;
  const bool trial = ident && wc->ident_ok != s->gen;
  if (trial && wc->ident_trial != 0) ident = false;
  const int seq = next_seq(s);
  // search blocks: one wave per window bound (2 per tile); key-stream blocks:
  // 2048 keys each, capped at the streaming grid.  A Pull checks its keys
  // inside k_resolve_apply, so on trusted windows it is one launch.
  const unsigned nsearch = trusted ? 0u : (unsigned)((2 * ntiles + kBlock / 64 - 1) / (kBlock / 64));
  const unsigned nval = op == PSG_PULL || ident ? 0u : grid_n(n, (uint64_t)kBlock * 8);
  // a validated Push on trusted windows also finds the tiles that are
  // stretches of the store (k_validate_windows, chunk_ok); PSG_RA_MIDENT=0:
  // never (A/B).  The flags live in one per-store array: its requests are
  // stream-ordered, each kernel reads only the marks of its own seq.
  static const bool mident_on = [] {
    const char* e = getenv("PSG_RA_MIDENT");
    return e ? atoi(e) != 0 : true;
  }();
  // (the array grows with the window-cache entries, win_entry: never here,
  // where a first stretch-tile request would wait for an allocation)
  const bool mident = mident_on && nval > 0 && nsearch == 0 && nt == 1024 && s->chunk_cap >= ntiles;
  // ... and resolves the tiles that are subsets of their windows there too
  // (k_validate_code; PSG_RA_CODED=0: the stretch check alone, A/B)
  static const bool coded_on = [] {
    const char* e = getenv("PSG_RA_CODED");
    return e ? atoi(e) != 0 : true;
  }();
  // the entry's lane codes (k_validate_code), kept with its windows and
  // verified by every request that uses them: allocated for the first Push
  // that validates coded tiles on it (without them, the stretch check alone)
  if (mident && coded_on && !wc->codes &&
      hipMalloc(&wc->codes, wc->cap_tiles * 1024 * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    wc->codes = nullptr;
  }
  const bool coded_ran = mident && coded_on && wc->codes;
  // the tiles the coded validation sorts as stretch or coded go to the lean
  // apply (k_tile_apply) while this list's last attempt left no general tile
  // against this K; f32 values (PSG_RA_LEAN=0: k_resolve_apply<MI>, A/B)
  static const bool lean_on = [] {
    const char* e = getenv("PSG_RA_LEAN");
    return e ? atoi(e) != 0 : true;
  }();
  const bool lean = lean_on && coded_ran && DT == PSG_F32 && (op & PSG_PUSH) && wc->lean_fail != s->gen;
  // A lean Push of a list that equals its verified copy needs no validation
  // pass against the store: k_list_check compares it with the copy (16 B per
  // key against 8 / density + 1 of store keys and lane codes) and takes the
  // tiles' kinds from their windows.  The copy is kept by a learning request
  // (k_validate_code writes the keys it validates) and holds while K keeps the
  // generation it was validated against.  PSG_RA_VL=0: never (A/B).
  static const bool vl_on = [] {
    const char* e = getenv("PSG_RA_VL");
    return e ? atoi(e) != 0 : true;
  }();
  const bool vl_ok = vl_on && lean && wc->vl_fail != s->gen;
  if (vl_ok && !wc->copy) {
    // (no request in flight reads an absent copy)
    if (hipMalloc(&wc->copy, wc->cap_tiles * 4096 * sizeof(uint64_t)) == hipSuccess) {
      wc->copy_cap = wc->cap_tiles * 4096;
      wc->copy_gen = 0;
    } else {
      (void)hipGetLastError();
      wc->copy = nullptr;
    }
  }
  const bool use_vl = vl_ok && wc->copy && wc->copy_cap >= n && wc->copy_gen == s->gen;
  const bool learn = vl_ok && wc->copy && wc->copy_cap >= n && !use_vl;
  if (use_vl) {
    // PSG_LC_BPC (A/B): blocks per CU (default 8); PSG_LC_NT=1: non-temporal loads
    static const int lc_bpc = [] {
      const char* e = getenv("PSG_LC_BPC");
      const int v = e ? atoi(e) : 0;
      return v >= 1 && v <= 32 ? v : 8;
    }();
    static const bool lc_nt = [] {
      const char* e = getenv("PSG_LC_NT");
      return e && atoi(e) != 0;
    }();
    const unsigned gl = std::min<unsigned>(grid_n(n, (uint64_t)kBlock * 4 * kIdU),
                                           (unsigned)(max_stream_blocks() / 8) * (unsigned)lc_bpc);
    const int lvec = aligned16(q) && aligned16(wc->copy) ? 1 : 0;
    if (lc_nt)
      k_list_check<1><<<gl, kBlock, 0, st>>>(q, wc->copy, n, win, s->gen, s->reject_dev, seq, lvec,
                                             tile_words(s, s->ring_next));
    else
      k_list_check<0><<<gl, kBlock, 0, st>>>(q, wc->copy, n, win, s->gen, s->reject_dev, seq, lvec,
                                             tile_words(s, s->ring_next));
    s->counters[PSG_CTR_LISTS]++;
  } else if (coded_ran) {
    const unsigned cus = (unsigned)(max_stream_blocks() / 8);
    // PSG_VC_BPC (A/B): blocks per CU in the grid (0: one block per tile)
    static const int vc_bpc = [] {
      const char* e = getenv("PSG_VC_BPC");
      return e ? atoi(e) : 2;
    }();
    const unsigned gcode = (unsigned)(vc_bpc > 0 ? std::min<uint64_t>(ntiles, (uint64_t)cus * vc_bpc) : ntiles);
    k_validate_code<<<gcode, 1024, 0, st>>>(q, n, s->keys, s->size, win, s->gen, s->key_begin, s->key_end,
                                            s->reject_dev, seq, aligned16(q) ? 1 : 0, tile_words(s, s->ring_next),
                                            wc->codes, learn ? wc->copy : nullptr);
    s->counters[PSG_CTR_CODED]++;
  } else if (nsearch + nval > 0)
    k_validate_windows<<<nsearch + nval, kBlock, 0, st>>>(q, n, s->keys, s->size, win, s->gen, tile, nsearch,
                                                         s->key_begin, s->key_end, s->reject_dev, seq,
                                                         aligned16(q) ? 1 : 0,
                                                         mident ? (int*)tile_words(s, s->ring_next) : nullptr);
  rec->ticket = ++s->next_ticket;
  if (ident && trial) wc->ident_trial = rec->ticket;
  rec->op = op;
  rec->q = q;
  rec->n = n;
  rec->vals = vals;
  rec->out = out;
  rec->ring = s->ring_next;
  s->ring_next = (s->ring_next + 1) % kRing;
  rec->tag = next_tag(s);
  rec->wc = (int)(wc - s->wc);
  rec->stream = st;
  rec->ident = ident ? 1 : 0;
  rec->mident = mident ? 1 : 0;
  rec->nt = nt;
  rec->seq = seq;
  rec->tw_ring = rec->ring;  // (the slot the validation above wrote: ring_next then)
  rec->lean = lean ? 1 : 0;
  rec->vl = use_vl ? 1 : (learn ? 2 : 0);
  if (learn) wc->learn_ticket = rec->ticket;
  s->counters[ident ? PSG_CTR_IDENT : PSG_CTR_FUSED]++;
  if (lean) {
    s->counters[PSG_CTR_LEAN]++;
    switch (op) {
      case PSG_PUSH: launch_tile_apply<DT, PSG_PUSH>(s, n, vals, out, win, *rec, st); break;
      default: launch_tile_apply<DT, PSG_PUSH | PSG_PULL>(s, n, vals, out, win, *rec, st); break;
    }
  } else if (ident) {
    switch (op) {
      case PSG_PUSH: launch_ident<DT, PSG_PUSH>(s, q, n, vals, out, win, *rec, st); break;
      case PSG_PULL: launch_ident<DT, PSG_PULL>(s, q, n, vals, out, win, *rec, st); break;
      default: launch_ident<DT, PSG_PUSH | PSG_PULL>(s, q, n, vals, out, win, *rec, st); break;
    }
  } else {
    switch (op) {
      case PSG_PUSH: launch_apply<DT, PSG_PUSH>(s, q, n, vals, out, win, *rec, st); break;
      case PSG_PULL: launch_apply<DT, PSG_PULL>(s, q, n, vals, out, win, *rec, st); break;
      default: launch_apply<DT, PSG_PUSH | PSG_PULL>(s, q, n, vals, out, win, *rec, st); break;
    }
  }
  PSG_HIP(hipGetLastError());
  // a synchronous Pull's reply is read by whoever the caller answers (a copy
  // engine, the host, another stream): behind the kernel an event of the ring
  // slot is recorded, and the reply is handed out once it has completed
  // (stream_done's semantics) — a poll instead of a stream synchronisation
  // (PSG_PULL_LAND=0: the synchronisation, A/B).  A request in flight skips
  // it: psg_store_wait synchronises its stream once instead.
  static const int land_on = [] {
    const char* e = getenv("PSG_PULL_LAND");
    return e ? atoi(e) : 1;
  }();
  rec->want_land = want_land && (op & PSG_PULL);
  rec->land = 0;
  if (rec->want_land && land_on && sync_poll() && s->land_ev[rec->ring]) {
    PSG_HIP(hipEventRecord(s->land_ev[rec->ring], st));
    rec->land = 1;
  }
  return PSG_OK;
}

// Wait for a fused request's completion word; after 2 ms (a long request, or a
// fault) synchronise the stream, which also reports any error.
// PSG_SYNC_POLL=0 always synchronises the stream first (A/B).
static int wait_landed(psg_store* s, const InflightReq& r);

static int wait_word(psg_store* s, const InflightReq& r, uint32_t* flags) {
  const volatile uint32_t* w = s->ring_host + r.ring;
  bool synced = false;
  if (!sync_poll()) {
    PSG_HIP(hipStreamSynchronize(r.stream));
    synced = true;
  }
  auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; ++spin) {
    const uint32_t v = *w;
    if ((v >> 8) == r.tag) {
      std::atomic_thread_fence(std::memory_order_acquire);
      *flags = v & 0xffu;
      return PSG_OK;
    }
    if (synced) break;
    if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
      PSG_HIP(hipStreamSynchronize(r.stream));
      synced = true;
    }
    __builtin_ia32_pause();
  }
  set_error("SORTED store: request %llu finished without its completion word", (unsigned long long)r.ticket);
  return PSG_ERR_HIP;
}

// A Pull's reply in memory: its landed word (launch_fused), else the stream
// synchronised.  Called once the request needs no follow-up (the follow-ups
// end with a synchronisation of their own).
static int wait_landed(psg_store* s, const InflightReq& r) {
  if (!(r.op & PSG_PULL)) return PSG_OK;
  if (!r.want_land) {  // in flight: psg_store_wait synchronises its stream
    bool known = false;
    for (hipStream_t u : s->unlanded) known = known || u == r.stream;
    if (!known) s->unlanded.push_back(r.stream);
    return PSG_OK;
  }
  if (r.land) return poll_event(s->land_ev[r.ring]);
  PSG_HIP(hipStreamSynchronize(r.stream));
  return PSG_OK;
}

// After a fused request's word: the window-cache policy, then what the word
// asks of the host.  A key outside the shard rejects the request (nothing was
// written); keys out of order or repeated take the order-preserving path (the
// fused kernels wrote nothing but, for a Pull, its reply, which that path
// rewrites); absent keys are inserted and the request applied to them.
template <int DT>
static int reap_t(psg_store* s, uint64_t upto, uint64_t own, int* own_rc);

// An identity request's verdict for its key list: a completed one proves the
// list a stretch of this K; either way the attempt is no longer in flight.
static void end_ident(psg_store* s, const InflightReq& r, bool completed_as_one) {
  psg_store::WinCache& wc = s->wc[r.wc];
  if (!r.ident || wc.q != r.q || wc.n != r.n) return;
  if (wc.ident_trial == r.ticket) wc.ident_trial = 0;
  if (completed_as_one) wc.ident_ok = s->gen;
}

template <int DT>
static int finish(psg_store* s, const InflightReq& r, uint32_t f) {
  psg_store::WinCache& wc = s->wc[r.wc];
  end_ident(s, r, !(f & (W_NOTIDENT | W_RANGE)));
  const bool mine = wc.q == r.q && wc.n == r.n;
  if (f & W_NOTLIST) {
    // not its list's verified copy after all (the caller rewrote the keys): it
    // wrote nothing.  No verified-copy attempt on this list until K changes;
    // the request runs again with the full validation, to completion (kPending,
    // which its word raised, is cleared first so it is not gated).
    if (mine) {
      wc.copy_gen = 0;
      wc.vl_fail = s->gen;
    }
    s->counters[PSG_CTR_NOTLIST]++;
    PSG_HIP(hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream));
    InflightReq r2;
    PSG_TRY(launch_fused<DT>(s, r.op, r.q, r.n, r.vals, r.out, r.stream, &r2, r.want_land != 0));
    PSG_REQUIRE(r2.vl != 1, PSG_ERR_HIP, "SORTED store: verified-copy request replayed as one");
    s->inflight.push_back(r2);
    int rc2 = PSG_OK;
    const int rc = reap_t<DT>(s, r2.ticket, r2.ticket, &rc2);
    return rc != PSG_OK ? rc : rc2;
  }
  // a learning request that completed with every tile served lean: its copy of
  // the list is now the verified copy for this K (the last learner's only)
  if (r.vl == 2 && mine && wc.learn_ticket == r.ticket &&
      !(f & (W_RANGE | W_UNSORTED | W_MISSING | W_WINMISS | W_PARTIAL | W_NOTIDENT)))
    wc.copy_gen = s->gen;
  if (f & W_NOTIDENT) {
    // not an identity request after all: it wrote nothing to the store (a
    // Pull, only its reply).  No identity attempt on this key list until K
    // changes; the request runs again on the general path, to completion
    // (kPending, which its word raised, is cleared first so it is not gated).
    if (wc.q == r.q && wc.n == r.n) wc.ident_fail = s->gen;
    s->counters[PSG_CTR_NOTIDENT]++;
    PSG_HIP(hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream));
    InflightReq r2;
    PSG_TRY(launch_fused<DT>(s, r.op, r.q, r.n, r.vals, r.out, r.stream, &r2, r.want_land != 0));
    PSG_REQUIRE(!r2.ident, PSG_ERR_HIP, "SORTED store: identity request replayed as one");
    s->inflight.push_back(r2);
    int rc2 = PSG_OK;
    const int rc = reap_t<DT>(s, r2.ticket, r2.ticket, &rc2);
    return rc != PSG_OK ? rc : rc2;
  }
  if (f & W_PARTIAL) {
    // k_tile_apply served the stretch and coded tiles and left the general
    // ones: k_resolve_apply<MI> for the same request (same seq: it reads the
    // request's tile words and takes every tile not general as done), to
    // completion; no speculation on this list until K changes.  kPending,
    // which the word raised, is cleared first so the follow-up is not gated.
    s->counters[PSG_CTR_LEAN_PARTIAL]++;
    if (wc.q == r.q && wc.n == r.n) wc.lean_fail = s->gen;
    PSG_HIP(hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream));
    InflightReq r2 = r;
    r2.ticket = ++s->next_ticket;
    r2.ring = s->ring_next;
    s->ring_next = (s->ring_next + 1) % kRing;
    r2.tag = next_tag(s);
    r2.lean = 2;  // (the follow-up: general tiles only)
    r2.land = 0;
    Win* win = static_cast<Win*>(wc.win);
    switch (r.op) {
      case PSG_PUSH: launch_apply<DT, PSG_PUSH>(s, r.q, r.n, r.vals, r.out, win, r2, r.stream); break;
      default: launch_apply<DT, PSG_PUSH | PSG_PULL>(s, r.q, r.n, r.vals, r.out, win, r2, r.stream); break;
    }
    PSG_HIP(hipGetLastError());
    if (r2.want_land && sync_poll() && s->land_ev[r2.ring]) {
      PSG_HIP(hipEventRecord(s->land_ev[r2.ring], r.stream));
      r2.land = 1;
    }
    s->inflight.push_back(r2);
    int rc2 = PSG_OK;
    const int rc = reap_t<DT>(s, r2.ticket, r2.ticket, &rc2);
    return rc != PSG_OK ? rc : rc2;
  }
  if (wc.q == r.q && wc.n == r.n) {
    if (f & W_WINMISS) {
      wc.trusted = 0;
      wc.strikes++;
    } else if (wc.strikes < 2 && !(f & (W_RANGE | W_UNSORTED))) {
      wc.trusted = (int)s->gen;  // trusted while K keeps this generation
    }
  }
  if (f & W_RANGE)
    PSG_REQUIRE(false, PSG_ERR_RANGE, "request key outside the store range [%llu, %llu) (nothing applied)",
                (unsigned long long)s->key_begin, (unsigned long long)s->key_end);
  if (f & W_UNSORTED) return general_request<DT>(s, r.op, r.q, r.vals, r.out, r.n, r.stream);
  if (!(f & W_MISSING)) return wait_landed(s, r);
  // the fused pass kept no slots: resolve again (the keys have not changed)
  // so the insert and the fixup know which keys were absent
  PSG_TRY(ensure_slots(s, r.n));
  PSG_TRY(launch_resolve(s, r.q, r.n, s->slots, r.stream));
  PSG_TRY(insert_missing(s, r.q, r.n, r.stream));
  PSG_TRY(launch_resolve(s, r.q, r.n, s->slots2, r.stream));
  PSG_TRY(run_fixup<DT>(s, r.op, r.vals, r.out, r.n, r.stream));
  PSG_TRY(read_flags(s, r.stream));
  PSG_REQUIRE(s->flags_host[F_MISSING] == 0, PSG_ERR_HIP, "SORTED store: keys still absent after insert");
  return PSG_OK;
}

// The status of a reaped request: returned to its synchronous caller (own),
// else kept for psg_store_wait (the first failure).
static void note(psg_store* s, uint64_t ticket, int rc, uint64_t own, int* own_rc) {
  if (ticket == own) {
    *own_rc = rc;
    return;
  }
  if (rc != PSG_OK && s->async_rc == PSG_OK) {
    s->async_rc = rc;
    s->async_msg = psg_last_error();
  }
}

// Reap the fused requests in flight, in launch order, up to ticket `upto`.
// A request whose word asks for the host's follow-up has raised kPending, so
// every request launched after it wrote nothing and reports W_GATED: those
// are waited for, the follow-up runs, kPending is cleared, and the gated
// requests are replayed in their order, each to completion — the store sees
// exactly the requests' sequence.
template <int DT>
static int reap_t(psg_store* s, uint64_t upto, uint64_t own, int* own_rc) {
  auto replay = [&](const InflightReq& g) {
    end_ident(s, g, false);  // gated: no verdict
    InflightReq r2;
    int rc = launch_fused<DT>(s, g.op, g.q, g.n, g.vals, g.out, g.stream, &r2, g.want_land != 0);
    if (rc == PSG_OK) {
      s->inflight.push_back(r2);
      int rc2 = PSG_OK;
      rc = reap_t<DT>(s, r2.ticket, r2.ticket, &rc2);
      if (rc == PSG_OK) rc = rc2;
    }
    note(s, g.ticket, rc, own, own_rc);
  };
  while (!s->inflight.empty() && s->inflight.front().ticket <= upto) {
    const InflightReq r = s->inflight.front();
    s->inflight.pop_front();
    uint32_t f = 0;
    int rc = wait_word(s, r, &f);
    if (rc != PSG_OK) {
      note(s, r.ticket, rc, own, own_rc);
      // a lost word: the stream is broken.  The arrival counters of this slot
      // and of the requests behind it were never zeroed by a completing block
      // — a slot used again would start from a stale count — so every set is
      // zeroed (and the gate word cleared) once the device is idle.
      // Only the streams of this store's requests are waited for (other
      // stores' and the application's work may run on): the failed request's
      // and those still in flight behind it.
      std::vector<hipStream_t> sts{r.stream};
      for (const InflightReq& g : s->inflight)
        if (std::find(sts.begin(), sts.end(), g.stream) == sts.end()) sts.push_back(g.stream);
      s->inflight.clear();
      for (auto& c : s->wc) c.ident_trial = 0;
      bool idle = true;
      for (hipStream_t u : sts) idle = idle && hipStreamSynchronize(u) == hipSuccess;
      if (idle) {
        constexpr size_t kCtrBytes = (size_t)kRing * (kArriveShards + 1) * kArriveStride * sizeof(uint64_t);
        (void)hipMemsetAsync(s->done_ctr, 0, kCtrBytes, r.stream);
        (void)hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream);
        (void)hipStreamSynchronize(r.stream);
      }
      return rc;
    }
    if (f & W_GATED) {  // gated by a follow-up already done (or an earlier failure)
      PSG_HIP(hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream));
      replay(r);
      continue;
    }
    const bool follow = !(f & W_RANGE) && (f & (W_MISSING | W_UNSORTED | W_NOTIDENT | W_NOTLIST));
    if (!follow) {
      note(s, r.ticket, finish<DT>(s, r, f), own, own_rc);
      continue;
    }
    std::vector<std::pair<InflightReq, uint32_t>> later;
    for (const InflightReq& g : s->inflight) {
      uint32_t gf = 0;
      rc = wait_word(s, g, &gf);
      if (rc != PSG_OK) {
        note(s, g.ticket, rc, own, own_rc);
        s->inflight.clear();
        for (auto& c : s->wc) c.ident_trial = 0;
        return rc;
      }
      later.emplace_back(g, gf);
    }
    s->inflight.clear();
    note(s, r.ticket, finish<DT>(s, r, f), own, own_rc);
    PSG_HIP(hipMemsetAsync(s->reject_dev + kPending, 0, sizeof(int), r.stream));
    for (auto& [g, gf] : later) {
      if (gf & W_GATED) replay(g);
      else note(s, g.ticket, finish<DT>(s, g, gf), own, own_rc);  // (cannot happen: kPending was up)
    }
  }
  return PSG_OK;
}

static int reap(psg_store* s, uint64_t upto, uint64_t own, int* own_rc) {
  switch (s->dtype) {
    case PSG_F32: return reap_t<PSG_F32>(s, upto, own, own_rc);
    case PSG_F64: return reap_t<PSG_F64>(s, upto, own, own_rc);
    case PSG_F16: return reap_t<PSG_F16>(s, upto, own, own_rc);
    default: return reap_t<PSG_BF16>(s, upto, own, own_rc);
  }
}

// Every request in flight complete (their failures kept for psg_store_wait).
static int drain(psg_store* s) {
  if (s->inflight.empty()) return PSG_OK;
  int unused = PSG_OK;
  return reap(s, ~0ull, 0, &unused);
}

// PSG_SORTED_FUSED=0: the two-pass form (resolve to slots, then k_slots), for A/B runs.
static bool sorted_fused() {
  static const bool on = [] {
    const char* e = getenv("PSG_SORTED_FUSED");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

static int launch_fused_any(psg_store* s, int op, const uint64_t* q, uint64_t n, const void* vals, void* out,
                            hipStream_t st, InflightReq* rec, bool want_land) {
  switch (s->dtype) {
    case PSG_F32: return launch_fused<PSG_F32>(s, op, q, n, vals, out, st, rec, want_land);
    case PSG_F64: return launch_fused<PSG_F64>(s, op, q, n, vals, out, st, rec, want_land);
    case PSG_F16: return launch_fused<PSG_F16>(s, op, q, n, vals, out, st, rec, want_land);
    default: return launch_fused<PSG_BF16>(s, op, q, n, vals, out, st, rec, want_land);
  }
}

// The two-pass form (an empty store, or the A/B switch), synchronous: the
// flags are read before the slot pass writes anything.
static int sorted_twopass(psg_store* s, int op, const uint64_t* q, const void* vals, void* out, uint64_t n,
                          hipStream_t st) {
  PSG_TRY(ensure_slots(s, n));
  PSG_TRY(launch_resolve(s, q, n, s->slots, st));
  PSG_TRY(read_flags(s, st));
  PSG_REQUIRE(!s->flags_host[F_RANGE], PSG_ERR_RANGE, "request key outside the store range [%llu, %llu)",
              (unsigned long long)s->key_begin, (unsigned long long)s->key_end);
  if (s->flags_host[F_UNSORTED]) return general_dispatch(s, op, q, vals, out, n, st);
  PSG_TRY(slot_request(s->dtype, op, s->vals, s->slots, vals, out, n, st));
  PSG_TRY(read_flags(s, st));
  if (s->flags_host[F_MISSING] == 0) return PSG_OK;
  PSG_TRY(insert_missing(s, q, n, st));
  PSG_TRY(launch_resolve(s, q, n, s->slots2, st));
  switch (s->dtype) {
    case PSG_F32: PSG_TRY(run_fixup<PSG_F32>(s, op, vals, out, n, st)); break;
    case PSG_F64: PSG_TRY(run_fixup<PSG_F64>(s, op, vals, out, n, st)); break;
    case PSG_F16: PSG_TRY(run_fixup<PSG_F16>(s, op, vals, out, n, st)); break;
    default: PSG_TRY(run_fixup<PSG_BF16>(s, op, vals, out, n, st)); break;
  }
  PSG_TRY(read_flags(s, st));
  PSG_REQUIRE(s->flags_host[F_MISSING] == 0, PSG_ERR_HIP, "SORTED store: keys still absent after insert");
  return PSG_OK;
}

// Resolve q to slots (psg_store_resolve), inserting absent keys when asked.
// A slot list must name each key once, in ascending order (the cached-slot
// kernels update each slot from one lane).
static int sorted_resolve(psg_store* s, const uint64_t* q, uint64_t n, bool insert, hipStream_t st) {
  PSG_TRY(ensure_slots(s, n));
  PSG_TRY(launch_resolve(s, q, n, s->slots, st));
  PSG_TRY(read_flags(s, st));
  PSG_TRY(check_request_flags(s));
  if (s->flags_host[F_MISSING] == 0 || !insert) return PSG_OK;
  PSG_TRY(insert_missing(s, q, n, st));
  PSG_TRY(launch_resolve(s, q, n, s->slots, st));
  PSG_TRY(read_flags(s, st));
  PSG_REQUIRE(s->flags_host[F_MISSING] == 0, PSG_ERR_HIP, "SORTED store: keys still absent after insert");
  return PSG_OK;
}

template <int DT>
static int run_dense_keyed(psg_store* s, int op, const uint64_t* keys, const void* vals, void* out,
                           uint64_t n, hipStream_t st) {
  using T = typename Elem<DT>::T;
  unsigned g = grid_n(n, kBlock);
  const int seq = next_seq(s);
  // validate the whole request first; the apply writes nothing if it failed
  k_validate_keys<<<g, kBlock, 0, st>>>(keys, n, s->key_begin, s->capacity, s->reject_dev, seq, s->flags);
  switch (op) {
    case PSG_PUSH:
      k_dense_keyed<DT, PSG_PUSH><<<g, kBlock, 0, st>>>((T*)s->vals, s->key_begin, s->capacity, keys,
                                                        (const T*)vals, (T*)out, n, s->reject_dev, seq);
      break;
    case PSG_PULL:
      k_dense_keyed<DT, PSG_PULL><<<g, kBlock, 0, st>>>((T*)s->vals, s->key_begin, s->capacity, keys,
                                                        (const T*)vals, (T*)out, n, s->reject_dev, seq);
      break;
    default:
      k_dense_keyed<DT, PSG_PUSH | PSG_PULL><<<g, kBlock, 0, st>>>(
          (T*)s->vals, s->key_begin, s->capacity, keys, (const T*)vals, (T*)out, n, s->reject_dev, seq);
  }
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// One request, synchronously: its status is the return value.
static int handle_sync(psg_store* s, int flags, const uint64_t* keys, uint64_t first_key, const void* vals,
                       void* out, uint64_t n, hipStream_t st) {
  PSG_TRY(drain(s));
  if (s->kind == PSG_STORE_DENSE) {
    if (!keys) {
      PSG_REQUIRE(first_key >= s->key_begin && first_key - s->key_begin <= s->capacity &&
                      n <= s->capacity - (first_key - s->key_begin),
                  PSG_ERR_RANGE, "dense request [%llu, +%llu) outside store slots [%llu, +%llu)",
                  (unsigned long long)first_key, (unsigned long long)n,
                  (unsigned long long)s->key_begin, (unsigned long long)s->capacity);
      char* base = (char*)s->vals + (first_key - s->key_begin) * s->esize;
      return dense_request(s->dtype, flags, base, vals, out, n, st);
    }
    reset_flags(s);
    int rc;
    switch (s->dtype) {
      case PSG_F32: rc = run_dense_keyed<PSG_F32>(s, flags, keys, vals, out, n, st); break;
      case PSG_F64: rc = run_dense_keyed<PSG_F64>(s, flags, keys, vals, out, n, st); break;
      case PSG_F16: rc = run_dense_keyed<PSG_F16>(s, flags, keys, vals, out, n, st); break;
      default: rc = run_dense_keyed<PSG_BF16>(s, flags, keys, vals, out, n, st); break;
    }
    PSG_TRY(rc);
    PSG_TRY(read_flags(s, st));
    PSG_REQUIRE(!s->flags_host[F_RANGE], PSG_ERR_RANGE,
                "request key outside the DENSE store slots [%llu, +%llu) (nothing applied)",
                (unsigned long long)s->key_begin, (unsigned long long)s->capacity);
    // keys out of order or repeated: applied in arrival order (KVApp.h:446-454)
    if (s->flags_host[F_UNSORTED]) return general_dispatch(s, flags, keys, vals, out, n, st);
    return PSG_OK;
  }
  PSG_REQUIRE(keys, PSG_ERR_INVALID, "SORTED store needs explicit keys");
  if (!sorted_fused() || s->size == 0) return sorted_twopass(s, flags, keys, vals, out, n, st);
  InflightReq rec;
  PSG_TRY(launch_fused_any(s, flags, keys, n, vals, out, st, &rec, true));
  s->inflight.push_back(rec);
  int own_rc = PSG_OK;
  PSG_TRY(reap(s, rec.ticket, rec.ticket, &own_rc));
  return own_rc;
}

// ---- a run of queued Pushes on one key list (psg_frames.hip) --------------
// PSG_FRAMES=0: every run is served request by request (A/B).
static bool frames_on() {
  static const bool on = [] {
    const char* e = getenv("PSG_FRAMES");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

// The k requests one after the other, each to completion: the reference's
// sequence, and the fallback of every run the one-pass forms do not cover.
// (psg_store_run_status: a request refused for a key outside the range is
// recorded and the run goes on; any other failure stops it)
static int one_status(psg_store* s, int k, int j, int rc) {
  if (!s->run_status || rc == PSG_OK) return rc;
  s->run_status[j] = rc;
  if (rc == PSG_ERR_RANGE) return PSG_OK;
  for (int i = j + 1; i < k; ++i) s->run_status[i] = rc;
  return rc;
}

static int frames_one_by_one(psg_store* s, const uint64_t* const* keys, uint64_t first_key,
                             const void* const* vals, int k, uint64_t n, hipStream_t st) {
  for (int j = 0; j < k; ++j)
    PSG_TRY(one_status(s, k, j, handle_sync(s, PSG_PUSH, keys ? keys[j] : nullptr, first_key, vals[j], nullptr, n, st)));
  return PSG_OK;
}

static void count_run(psg_store* s, int k) {
  s->counters[PSG_CTR_RUNS]++;
  s->counters[PSG_CTR_RUN_FRAMES] += (uint64_t)k;
}

// Runs on a SORTED store: (1) the lists are a stretch K[D, D + n) of the
// store — frames_base, frames_check of every list against it, frames_apply,
// one flag read; (2) else list 0 resolved to slots (no key absent, in range,
// ascending), lists 1..k-1 checked against list 0, frames_slots; (3) else one
// by one.  A failed check wrote nothing (the apply kernels read its word
// first), so every fallback starts from the store the run found.
static int frames_sorted(psg_store* s, const uint64_t* const* keys, const void* const* vals, int k, uint64_t n,
                         hipStream_t st, int* fused) {
  if (!sorted_fused() || s->size == 0 || n > s->size) return frames_one_by_one(s, keys, 0, vals, k, n, st);
  uint64_t* base = reinterpret_cast<uint64_t*>(s->reject_dev + kFramesBase);
  int* rej = s->reject_dev + kRejIdent;
  int seq = next_seq(s);
  reset_flags(s);
  PSG_TRY(frames_base(s->keys, s->size, keys[0], n, base, st));
  PSG_TRY(frames_check(s->keys, base, keys, 0, k, n, rej, seq, st));
  PSG_TRY(frames_apply(s->dtype, s->vals, s->size, vals, k, n, base, rej, seq, s->flags + F_MISSING, st));
  PSG_TRY(read_flags(s, st));
  if (!s->flags_host[F_MISSING]) {
    *fused = 1;
    count_run(s, k);
    return PSG_OK;
  }
  PSG_TRY(ensure_slots(s, n));
  PSG_TRY(launch_resolve(s, keys[0], n, s->slots, st));
  PSG_TRY(read_flags(s, st));
  const int* f = s->flags_host;
  if (f[F_MISSING] || f[F_RANGE] || f[F_UNSORTED]) return frames_one_by_one(s, keys, 0, vals, k, n, st);
  seq = next_seq(s);
  reset_flags(s);
  PSG_TRY(frames_check(keys[0], nullptr, keys, 1, k, n, rej, seq, st));
  PSG_TRY(frames_slots(s->dtype, s->vals, s->slots, vals, k, n, rej, seq, s->flags + F_MISSING, st));
  PSG_TRY(read_flags(s, st));
  if (s->flags_host[F_MISSING]) return frames_one_by_one(s, keys, 0, vals, k, n, st);
  *fused = 1;
  count_run(s, k);
  return PSG_OK;
}

// ---- a run of queued requests on interleaved lists (psg_runs.hip) ---------
// PSG_RUNS_STRIDED=0: psg_store_run never tries the strided pass (A/B).
static bool strided_on() {
  static const bool on = [] {
    const char* e = getenv("PSG_RUNS_STRIDED");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

static int run_one_by_one(psg_store* s, int k, const int* ops, const uint64_t* const* keys, const uint64_t* ns,
                          const void* const* vals, void* const* outs, hipStream_t st) {
  for (int j = 0; j < k; ++j)
    PSG_TRY(one_status(s, k, j,
                       handle_sync(s, ops[j], keys[j], 0, (ops[j] & PSG_PUSH) ? vals[j] : nullptr,
                                   (ops[j] & PSG_PULL) ? outs[j] : nullptr, ns[j], st)));
  return PSG_OK;
}

// The layout of a run from the slots of its lists' first keys, learnt from
// earlier strided runs (s->run_pos): every list known at this K generation in
// one period.  The passes verify every key against it, so a stale or wrong
// guess only costs a rejected pass.
static bool run_from_cache(psg_store* s, int k, const uint64_t* const* keys, const uint64_t* ns, RunDesc* d) {
  uint64_t pos[kMaxFrames];
  uint32_t P = 0;
  for (int j = 0; j < k; ++j) {
    int hit = -1;
    for (int e = 0; e < 64 && hit < 0; ++e) {
      const auto& c = s->run_pos[e];
      if (c.q == keys[j] && c.n == ns[j] && c.gen == s->gen && c.P) hit = e;
    }
    if (hit < 0) return false;
    if (P && s->run_pos[hit].P != P) return false;
    P = s->run_pos[hit].P;
    pos[j] = s->run_pos[hit].pos0;
    s->run_pos[hit].last_use = ++s->run_clock;
  }
  uint64_t D = UINT64_MAX, rows = 0;
  for (int j = 0; j < k; ++j) D = pos[j] < D ? pos[j] : D;
  memset(d, 0, sizeof(*d));
  memset(d->map, -1, sizeof(d->map));
  for (int j = 0; j < k; ++j) {
    const uint64_t p = pos[j] - D;
    if (p >= P || d->map[p] >= 0) return false;
    d->map[p] = (int8_t)j;
    if (ns[j] > rows) rows = ns[j];
    if (p + (uint64_t)P * (ns[j] - 1) >= s->size - D) return false;
  }
  d->D = D;
  d->P = P;
  d->rows = rows;
  d->cls = RUN_STRIDED;
  return true;
}

static void run_remember(psg_store* s, int k, const uint64_t* const* keys, const uint64_t* ns, const RunSeen& seen) {
  for (int j = 0; j < k; ++j) {
    int slot = -1;
    uint64_t oldest = UINT64_MAX;
    for (int e = 0; e < 64; ++e) {
      const auto& c = s->run_pos[e];
      if (c.q == keys[j] && c.n == ns[j]) {
        slot = e;
        break;
      }
      if (c.last_use < oldest) oldest = c.last_use, slot = e;
    }
    auto& c = s->run_pos[slot];
    c.q = keys[j];
    c.n = ns[j];
    c.pos0 = seen.pos[j];
    c.P = seen.d.P;
    c.gen = s->gen;
    c.last_use = ++s->run_clock;
  }
}

// One launch sequence tries both one-pass forms, each gated on the device by
// what run_classify found from the first keys, so the host waits once:
//   same list (every request a Push on one list starting at one slot):
//     frames_check + frames_apply, as psg_store_push_frames;
//   strided (distinct phases of one period): run_pass check + apply, or one
//     checked pass for a run without Pushes.
// A run whose lists a pass rejected wrote nothing and is served request by
// request (a same-list run first through frames_sorted's slot form).  A
// strided run whose lists the host already knows (run_from_cache) skips the
// classify kernel: its layout goes to the passes as a kernel argument.
static int run_sorted(psg_store* s, int k, const int* ops, const uint64_t* const* keys, const uint64_t* ns,
                      const void* const* vals, void* const* outs, hipStream_t st, int* served, bool hinted = true) {
  bool all_push = true, any_push = false, same_n = true;
  uint64_t total = 0, max_n = 0;
  int pl = -1;
  for (int j = 0; j < k; ++j) {
    all_push = all_push && ops[j] == PSG_PUSH;
    any_push = any_push || (ops[j] & PSG_PUSH);
    same_n = same_n && ns[j] == ns[0];
    total += ns[j];
    max_n = ns[j] > max_n ? ns[j] : max_n;
    if (pl < 0 && ns[j] >= 2) pl = j;
  }
  // (a request on its own is a strided pass only when the host knows its
  // list's place: a single phase of a learnt layout, which moves 8 P + 8 P + 12
  // B per key of lines against the general path's windows and search)
  bool try_same = k > 1 && all_push && same_n && ns[0] <= s->size;
  bool try_strided = strided_on() && pl >= 0 && total <= s->size;
  // a run with Pulls that was not strided at this K generation: the next few
  // are served one by one without a try (a run of Pushes always tries: the
  // same-list pass shares the launch)
  if (try_strided && !all_push && s->run_fail_gen == s->gen && s->run_fail_count > 0) {
    --s->run_fail_count;
    try_strided = false;
  }
  // a run of Pushes that could be either form tries the one the last run was
  // served as first (its other pass would only launch to find itself gated)
  bool hint_used = false;
  if (hinted && try_same && try_strided) {
    if (s->run_last == PSG_RUN_SAME_LIST) try_strided = false, hint_used = true;
    else if (s->run_last == PSG_RUN_STRIDED) try_same = false, hint_used = true;
  }
  if (!try_same && !try_strided) return run_one_by_one(s, k, ops, keys, ns, vals, outs, st);
  RunFrames f = {};
  f.lo = s->key_begin;
  f.hi = s->key_end;
  for (int j = 0; j < k; ++j) {
    f.q[j] = keys[j];
    f.v[j] = (ops[j] & PSG_PUSH) ? vals[j] : nullptr;
    f.o[j] = (ops[j] & PSG_PULL) ? outs[j] : nullptr;
    f.n[j] = ns[j];
    f.op[j] = ops[j];
  }
  RunDesc given;
  memset(&given, 0, sizeof(given));
  const bool cached = !try_same && try_strided && run_from_cache(s, k, keys, ns, &given);
  if (k == 1 && !cached) return run_one_by_one(s, k, ops, keys, ns, vals, outs, st);
  RunDesc* desc = cached ? nullptr : static_cast<RunDesc*>(s->run_desc);
  uint64_t* base = reinterpret_cast<uint64_t*>(s->reject_dev + kFramesBase);
  int* rej = s->reject_dev + kRejIdent;
  int* bad = s->reject_dev + kRejRun;
  const int seq = next_seq(s);
  reset_flags(s);
  if (!cached)
    PSG_TRY(run_classify(s->keys, s->size, f, k, try_strided ? pl : -1, try_same ? 1 : 0, desc, s->run_seen, base, st));
  if (try_same) {
    PSG_TRY(frames_check(s->keys, base, keys, 0, k, ns[0], rej, seq, st));
    PSG_TRY(frames_apply(s->dtype, s->vals, s->size, vals, k, ns[0], base, rej, seq, s->flags + F_MISSING, st));
  }
  if (try_strided) {
    if (any_push) {
      PSG_TRY(run_pass(RUN_CHECK, s->dtype, s->vals, s->keys, s->size, f, k, max_n, desc, given, bad, seq, nullptr,
                       st));
      PSG_TRY(run_pass(RUN_APPLY, s->dtype, s->vals, s->keys, s->size, f, k, max_n, desc, given, bad, seq,
                       s->flags + F_WINMISS, st));
    } else {
      PSG_TRY(run_pass(RUN_PULL_CHECKED, s->dtype, s->vals, s->keys, s->size, f, k, max_n, desc, given, bad, seq,
                       s->flags + F_WINMISS, st));
    }
  }
  PSG_TRY(read_flags(s, st));
  if (try_same && !s->flags_host[F_MISSING]) {
    *served = PSG_RUN_SAME_LIST;
    count_run(s, k);
    return PSG_OK;
  }
  if (try_strided && !s->flags_host[F_WINMISS]) {
    *served = PSG_RUN_STRIDED;
    if (k == 1) {
      s->counters[PSG_CTR_STRIDED_SINGLE]++;
    } else {
      s->counters[PSG_CTR_STRIDED_RUNS]++;
      s->counters[PSG_CTR_STRIDED_FRAMES] += (uint64_t)k;
    }
    if (!cached) run_remember(s, k, keys, ns, *s->run_seen);
    return PSG_OK;
  }
  if (cached) {
    // the lists moved (or their contents changed) since they were learnt:
    // forget them, and classify afresh (nothing was written)
    for (auto& c : s->run_pos)
      for (int j = 0; j < k; ++j)
        if (c.q == keys[j]) c.P = 0;
    return run_sorted(s, k, ops, keys, ns, vals, outs, st, served, hinted);
  }
  if (try_strided && !all_push) {
    s->run_fail_gen = s->gen;
    s->run_fail_count = 8;
  }
  // the hinted form did not hold: both, as an unhinted run (nothing was written)
  if (hint_used) return run_sorted(s, k, ops, keys, ns, vals, outs, st, served, false);
  if (try_same) {
    int fused = 0;
    PSG_TRY(frames_sorted(s, keys, vals, k, ns[0], st, &fused));
    if (fused) *served = PSG_RUN_SAME_LIST;
    return PSG_OK;
  }
  return run_one_by_one(s, k, ops, keys, ns, vals, outs, st);
}

static int frames_args(psg_store* s, const void* const* vals_host, int k) {
  PSG_REQUIRE(s && vals_host, PSG_ERR_INVALID, "push frames: null argument");
  PSG_REQUIRE(k >= 1 && k <= kMaxFrames, PSG_ERR_INVALID, "push frames: 1..%d frames, got %d", kMaxFrames, k);
  for (int j = 0; j < k; ++j) PSG_REQUIRE(vals_host[j], PSG_ERR_INVALID, "push frames: null vals of frame %d", j);
  return PSG_OK;
}

}  // namespace psg

using namespace psg;

extern "C" {

int psg_store_create(int kind, int dtype, uint64_t key_begin, uint64_t key_end, uint64_t capacity,
                     psg_store** out) {
  PSG_REQUIRE(out, PSG_ERR_INVALID, "psg_store_create: null out");
  *out = nullptr;
  PSG_REQUIRE(kind == PSG_STORE_DENSE || kind == PSG_STORE_SORTED, PSG_ERR_INVALID,
              "psg_store_create: bad kind %d", kind);
  const int es = dtype_size(dtype);
  PSG_REQUIRE(es > 0, PSG_ERR_UNSUPPORTED, "psg_store_create: bad dtype %d", dtype);
  PSG_REQUIRE(key_begin < key_end, PSG_ERR_INVALID, "psg_store_create: empty key range");
  if (kind == PSG_STORE_DENSE)
    PSG_REQUIRE(capacity > 0 && capacity <= key_end - key_begin, PSG_ERR_INVALID,
                "psg_store_create: DENSE capacity %llu does not fit the key range",
                (unsigned long long)capacity);
  psg_store* s = new psg_store();  // value-initialised: every plain field zero
  s->kind = kind;
  s->dtype = dtype;
  s->esize = es;
  s->key_begin = key_begin;
  s->key_end = key_end;
  (void)hipGetDevice(&s->device);
  auto fail = [&](int rc) {
    psg_store_destroy(s);
    return rc;
  };
  hipError_t e;
  if ((e = hipHostMalloc(&s->flags_host, F_NFLAGS * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail(hip_fail(e, "hipHostMalloc(flags)", __FILE__, __LINE__));
  if ((e = hipHostGetDevicePointer((void**)&s->flags, s->flags_host, 0)) != hipSuccess)
    return fail(hip_fail(e, "hipHostGetDevicePointer(flags)", __FILE__, __LINE__));
  memset(s->flags_host, 0, F_NFLAGS * sizeof(int));
  if ((e = hipHostMalloc((void**)&s->ring_host, kRing * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail(hip_fail(e, "hipHostMalloc(completion ring)", __FILE__, __LINE__));
  if ((e = hipHostGetDevicePointer((void**)&s->ring_dev, s->ring_host, 0)) != hipSuccess)
    return fail(hip_fail(e, "hipHostGetDevicePointer(completion ring)", __FILE__, __LINE__));
  memset(s->ring_host, 0, kRing * sizeof(uint32_t));  // completion words
  if ((e = hipEventCreateWithFlags(&s->done_ev, hipEventDisableTiming)) != hipSuccess)
    return fail(hip_fail(e, "hipEventCreate(completion)", __FILE__, __LINE__));
  for (int i = 0; i < kRing; ++i)
    if ((e = hipEventCreateWithFlags(&s->land_ev[i], hipEventDisableTiming)) != hipSuccess)
      return fail(hip_fail(e, "hipEventCreate(landed reply)", __FILE__, __LINE__));
  if ((e = hipMalloc((void**)&s->reject_dev, 64)) != hipSuccess ||
      (e = hipMemset(s->reject_dev, 0, 64)) != hipSuccess)
    return fail(hip_fail(e, "hipMalloc(reject words)", __FILE__, __LINE__));
  if ((e = hipMalloc(&s->run_desc, sizeof(RunDesc))) != hipSuccess ||
      (e = hipMemset(s->run_desc, 0, sizeof(RunDesc))) != hipSuccess)
    return fail(hip_fail(e, "hipMalloc(run layout)", __FILE__, __LINE__));
  if ((e = hipHostMalloc((void**)&s->run_seen, sizeof(RunSeen), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail(hip_fail(e, "hipHostMalloc(run layout seen)", __FILE__, __LINE__));
  memset(s->run_seen, 0, sizeof(RunSeen));
  constexpr size_t kCtrBytes = (size_t)kRing * (kArriveShards + 1) * kArriveStride * sizeof(uint64_t);
  if ((e = hipMalloc((void**)&s->done_ctr, kCtrBytes)) != hipSuccess ||
      (e = hipMemset(s->done_ctr, 0, kCtrBytes)) != hipSuccess)
    return fail(hip_fail(e, "hipMalloc(completion counters)", __FILE__, __LINE__));
  s->gen = 1;  // cached windows carry gen >= 1; zeroed entries never match
  if (kind == PSG_STORE_DENSE) {
    s->capacity = capacity;
    s->size = capacity;
    // a DENSE shard is what peers map for the xGMI exchange (psg_xgmi_create)
    if ((e = hipMalloc(&s->vals, ipc_alloc_bytes(capacity * es))) != hipSuccess)
      return fail(hip_fail(e, "hipMalloc(store values)", __FILE__, __LINE__));
    if ((e = hipMemset(s->vals, 0, capacity * es)) != hipSuccess)
      return fail(hip_fail(e, "hipMemset(store values)", __FILE__, __LINE__));
  } else {
    s->capacity = 0;
    s->size = 0;
    if (capacity > 0) {
      PSG_REQUIRE(capacity <= 0xfffffffeull, PSG_ERR_RANGE, "SORTED store capacity above 2^32-2");
      if ((e = hipMalloc(&s->vals, capacity * es)) != hipSuccess)
        return fail(hip_fail(e, "hipMalloc(store values)", __FILE__, __LINE__));
      if ((e = hipMalloc(&s->keys, (capacity + kKeyPad) * sizeof(uint64_t))) != hipSuccess)
        return fail(hip_fail(e, "hipMalloc(store keys)", __FILE__, __LINE__));
      s->capacity = capacity;
    }
  }
  // the memsets above ran on the null stream, which does not order with the
  // caller's non-blocking streams: done before any request can be enqueued
  if ((e = hipStreamSynchronize(nullptr)) != hipSuccess)
    return fail(hip_fail(e, "hipStreamSynchronize(null stream)", __FILE__, __LINE__));
  *out = s;
  return PSG_OK;
}

int psg_store_destroy(psg_store* s) {
  if (!s) return PSG_OK;
  (void)drain(s);
  if (s->vals) (void)hipFree(s->vals);
  if (s->keys) (void)hipFree(s->keys);
  if (s->slots) (void)hipFree(s->slots);
  if (s->slots2) (void)hipFree(s->slots2);
  if (s->wlo) (void)hipFree(s->wlo);
  if (s->gbuf) (void)hipFree(s->gbuf);
  if (s->chunk_ok) (void)hipFree(s->chunk_ok);
  if (s->flags_host) (void)hipHostFree(s->flags_host);
  if (s->ring_host) (void)hipHostFree(s->ring_host);
  if (s->reject_dev) (void)hipFree(s->reject_dev);
  if (s->run_desc) (void)hipFree(s->run_desc);
  if (s->run_seen) (void)hipHostFree(s->run_seen);
  if (s->done_ctr) (void)hipFree(s->done_ctr);
  if (s->done_ev) (void)hipEventDestroy(s->done_ev);
  for (hipEvent_t ev : s->land_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& c : s->wc) {
    if (c.win) (void)hipFree(c.win);
    if (c.codes) (void)hipFree(c.codes);
    if (c.copy) (void)hipFree(c.copy);
  }
  delete s;
  return PSG_OK;
}

int psg_store_get_info(psg_store* s, psg_store_info* info) {
  PSG_REQUIRE(s && info, PSG_ERR_INVALID, "psg_store_get_info: null argument");
  PSG_TRY(drain(s));  // a request in flight may still insert keys
  info->kind = s->kind;
  info->dtype = s->dtype;
  info->key_begin = s->key_begin;
  info->key_end = s->key_end;
  info->size = s->size;
  info->capacity = s->capacity;
  info->vals = s->vals;
  info->keys = s->keys;
  return PSG_OK;
}

int psg_store_counters(psg_store* s, uint64_t* out, int n) {
  PSG_REQUIRE(s && (out || n == 0) && n >= 0, PSG_ERR_INVALID, "psg_store_counters: bad arguments");
  PSG_TRY(drain(s));  // a request in flight may still fall back
  for (int i = 0; i < n; ++i) out[i] = i < PSG_NCOUNTERS ? s->counters[i] : 0;
  return PSG_OK;
}

int psg_store_clear(psg_store* s, psg_stream stream) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_clear: null store");
  PSG_TRY(drain(s));
  if (s->kind == PSG_STORE_DENSE) {
    PSG_HIP(hipMemsetAsync(s->vals, 0, s->capacity * s->esize, (hipStream_t)stream));
  } else {
    s->size = 0;
    s->gen++;
  }
  return PSG_OK;
}

static int handle_args(psg_store* s, int flags, const void* vals, void* out) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_handle: null store");
  PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "psg_store_handle: bad flags %d", flags);
  PSG_REQUIRE(!(flags & PSG_PUSH) || vals, PSG_ERR_INVALID, "push without vals");
  PSG_REQUIRE(!(flags & PSG_PULL) || out, PSG_ERR_INVALID, "pull without out buffer");
  return PSG_OK;
}

int psg_store_handle(psg_store* s, int flags, const uint64_t* keys, uint64_t first_key,
                     const void* vals, void* out, uint64_t n, psg_stream stream) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_handle: null store");
  PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "psg_store_handle: bad flags %d", flags);
  if (n == 0) return PSG_OK;
  PSG_TRY(handle_args(s, flags, vals, out));
  return handle_sync(s, flags, keys, first_key, vals, out, n, (hipStream_t)stream);
}

int psg_store_handle_async(psg_store* s, int flags, const uint64_t* keys, uint64_t first_key, const void* vals,
                           void* out, uint64_t n, psg_stream stream, uint64_t* ticket) {
  PSG_REQUIRE(s && ticket, PSG_ERR_INVALID, "psg_store_handle_async: null argument");
  *ticket = 0;
  PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "psg_store_handle_async: bad flags %d", flags);
  if (n == 0) return PSG_OK;
  PSG_TRY(handle_args(s, flags, vals, out));
  hipStream_t st = (hipStream_t)stream;
  // only a fused keyed request on a populated SORTED store runs in flight;
  // every other form completes here, in order behind the requests in flight
  if (s->kind != PSG_STORE_SORTED || !keys || !sorted_fused() || s->size == 0)
    return handle_sync(s, flags, keys, first_key, vals, out, n, st);
  if (!s->inflight.empty() && s->inflight.back().stream != st) PSG_TRY(drain(s));  // one stream at a time
  if (s->inflight.size() >= (size_t)kRing - 1) {
    int unused = PSG_OK;
    PSG_TRY(reap(s, s->inflight.front().ticket, 0, &unused));
  }
  InflightReq rec;
  PSG_TRY(launch_fused_any(s, flags, keys, n, vals, out, st, &rec, false));
  s->inflight.push_back(rec);
  *ticket = rec.ticket;
  // an identity trial is reaped before anything is launched behind it: if the
  // list is not a stretch it raises kPending, and every request launched
  // behind it would be gated and launched again
  if (rec.ident && s->wc[rec.wc].ident_trial == rec.ticket) {
    int unused = PSG_OK;
    PSG_TRY(reap(s, rec.ticket, 0, &unused));
  }
  return PSG_OK;
}

int psg_store_wait(psg_store* s, uint64_t ticket) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_wait: null store");
  int unused = PSG_OK;
  PSG_TRY(reap(s, ticket ? ticket : ~0ull, 0, &unused));
  // reaped Pulls' replies in memory: every stream they ran on (a caller that
  // switched streams drained the old one's requests into this list too)
  while (!s->unlanded.empty()) {
    hipStream_t st = s->unlanded.back();
    s->unlanded.pop_back();
    PSG_HIP(hipStreamSynchronize(st));
  }
  if (s->async_rc != PSG_OK) {
    const int rc = s->async_rc;
    s->async_rc = PSG_OK;
    set_error("%s", s->async_msg.c_str());
    return rc;
  }
  return PSG_OK;
}

int psg_store_resolve(psg_store* s, const uint64_t* keys, uint64_t n, int insert, uint32_t* slots,
                      psg_stream stream) {
  PSG_REQUIRE(s && slots, PSG_ERR_INVALID, "psg_store_resolve: null argument");
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(keys, PSG_ERR_INVALID, "psg_store_resolve: null keys");
  PSG_TRY(drain(s));
  hipStream_t st = (hipStream_t)stream;
  if (s->kind == PSG_STORE_DENSE) {
    reset_flags(s);
    k_dense_slots<<<grid_n(n, kBlock), kBlock, 0, st>>>(keys, n, s->key_begin, s->capacity, slots,
                                                         s->flags);
    PSG_HIP(hipGetLastError());
    PSG_TRY(read_flags(s, st));
    PSG_REQUIRE(!s->flags_host[F_UNSORTED], PSG_ERR_INVALID,
                "slot list keys are not strictly ascending (each key once)");
    PSG_REQUIRE(!s->flags_host[F_RANGE], PSG_ERR_RANGE, "key outside the DENSE store slots");
    return PSG_OK;
  }
  PSG_TRY(sorted_resolve(s, keys, n, insert != 0, st));
  PSG_HIP(hipMemcpyAsync(slots, s->slots, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return PSG_OK;
}

int psg_store_slots_stretch(psg_store* s, const uint32_t* slots, uint64_t n, uint64_t* first,
                            psg_stream stream) {
  PSG_REQUIRE(s && first, PSG_ERR_INVALID, "psg_store_slots_stretch: null argument");
  *first = UINT64_MAX;
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(slots, PSG_ERR_INVALID, "psg_store_slots_stretch: null slots");
  PSG_TRY(drain(s));
  hipStream_t st = (hipStream_t)stream;
  reset_flags(s);
  k_slots_stretch<<<grid_n(n, kBlock), kBlock, 0, st>>>(slots, n, s->flags);
  PSG_HIP(hipGetLastError());
  PSG_TRY(read_flags(s, st));
  if (s->flags_host[F_MISSING]) return PSG_OK;
  uint32_t s0 = 0;
  // on the caller's stream (a null-stream copy does not order with it)
  PSG_HIP(hipMemcpyAsync(&s0, slots, sizeof(s0), hipMemcpyDeviceToHost, st));
  PSG_HIP(hipStreamSynchronize(st));
  const uint64_t limit = s->kind == PSG_STORE_SORTED ? s->size : s->capacity;
  if (s0 != kNoSlot && (uint64_t)s0 <= limit && n <= limit - s0) *first = s0;
  return PSG_OK;
}

int psg_store_handle_stretch(psg_store* s, int flags, uint64_t first, const void* vals, void* out, uint64_t n,
                             psg_stream stream) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_handle_stretch: null store");
  PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "bad flags %d", flags);
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(!(flags & PSG_PUSH) || vals, PSG_ERR_INVALID, "push without vals");
  PSG_REQUIRE(!(flags & PSG_PULL) || out, PSG_ERR_INVALID, "pull without out buffer");
  PSG_TRY(drain(s));
  const uint64_t limit = s->kind == PSG_STORE_SORTED ? s->size : s->capacity;
  PSG_REQUIRE(first <= limit && n <= limit - first, PSG_ERR_RANGE,
              "psg_store_handle_stretch: slots [%llu, %llu) past the store's %llu", (unsigned long long)first,
              (unsigned long long)(first + n), (unsigned long long)limit);
  return dense_request(s->dtype, flags, static_cast<char*>(s->vals) + first * (uint64_t)s->esize, vals, out, n,
                       (hipStream_t)stream);
}

int psg_store_sync(psg_store* s, psg_stream stream) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_sync: null store");
  PSG_TRY(drain(s));
  return read_flags(s, (hipStream_t)stream);
}

int psg_store_handle_slots(psg_store* s, int flags, const uint32_t* slots, const void* vals,
                           void* out, uint64_t n, psg_stream stream) {
  PSG_REQUIRE(s, PSG_ERR_INVALID, "psg_store_handle_slots: null store");
  PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "bad flags %d", flags);
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(slots, PSG_ERR_INVALID, "null slots");
  PSG_REQUIRE(!(flags & PSG_PUSH) || vals, PSG_ERR_INVALID, "push without vals");
  PSG_REQUIRE(!(flags & PSG_PULL) || out, PSG_ERR_INVALID, "pull without out buffer");
  PSG_TRY(drain(s));
  return slot_request(s->dtype, flags, s->vals, slots, vals, out, n, (hipStream_t)stream);
}

int psg_store_push_frames(psg_store* s, const uint64_t* const* keys_host, uint64_t first_key,
                          const void* const* vals_host, int k, uint64_t n, psg_stream stream, int* fused_host) {
  if (fused_host) *fused_host = 0;
  PSG_TRY(frames_args(s, vals_host, k));
  if (keys_host)
    for (int j = 0; j < k; ++j) PSG_REQUIRE(keys_host[j], PSG_ERR_INVALID, "push frames: null keys of frame %d", j);
  if (n == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(drain(s));
  if (k == 1 || !frames_on()) return frames_one_by_one(s, keys_host, first_key, vals_host, k, n, st);
  int fused = 0;
  if (s->kind == PSG_STORE_DENSE) {
    if (keys_host) return frames_one_by_one(s, keys_host, first_key, vals_host, k, n, st);
    PSG_REQUIRE(first_key >= s->key_begin && first_key - s->key_begin <= s->capacity &&
                    n <= s->capacity - (first_key - s->key_begin),
                PSG_ERR_RANGE, "dense run [%llu, +%llu) outside store slots [%llu, +%llu)",
                (unsigned long long)first_key, (unsigned long long)n, (unsigned long long)s->key_begin,
                (unsigned long long)s->capacity);
    char* at = (char*)s->vals + (first_key - s->key_begin) * s->esize;
    PSG_TRY(frames_apply(s->dtype, at, s->capacity, vals_host, k, n, nullptr, nullptr, 0, s->flags + F_MISSING, st));
    fused = 1;
    count_run(s, k);
  } else {
    PSG_REQUIRE(keys_host, PSG_ERR_INVALID, "SORTED store needs explicit keys");
    PSG_TRY(frames_sorted(s, keys_host, vals_host, k, n, st, &fused));
  }
  if (fused_host) *fused_host = fused;
  return PSG_OK;
}

int psg_store_run(psg_store* s, int k, const int* ops, const uint64_t* const* keys, const uint64_t* ns,
                  const void* const* vals, void* const* outs, psg_stream stream, int* served) {
  if (served) *served = PSG_RUN_ONE_BY_ONE;
  PSG_REQUIRE(s && ops && keys && ns, PSG_ERR_INVALID, "psg_store_run: null argument");
  PSG_REQUIRE(k >= 1 && k <= kMaxFrames, PSG_ERR_INVALID, "psg_store_run: 1..%d requests, got %d", kMaxFrames, k);
  bool any_push = false, any_pull = false;
  for (int j = 0; j < k; ++j) {
    PSG_REQUIRE(ops[j] >= 1 && ops[j] <= 3, PSG_ERR_INVALID, "psg_store_run: bad flags %d of request %d", ops[j], j);
    PSG_REQUIRE(ns[j] == 0 || keys[j], PSG_ERR_INVALID, "psg_store_run: null keys of request %d", j);
    any_push = any_push || (ops[j] & PSG_PUSH);
    any_pull = any_pull || (ops[j] & PSG_PULL);
    PSG_REQUIRE(!(ops[j] & PSG_PUSH) || ns[j] == 0 || (vals && vals[j]), PSG_ERR_INVALID,
                "psg_store_run: push without vals (request %d)", j);
    PSG_REQUIRE(!(ops[j] & PSG_PULL) || ns[j] == 0 || (outs && outs[j]), PSG_ERR_INVALID,
                "psg_store_run: pull without out buffer (request %d)", j);
  }
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(drain(s));
  int sv = PSG_RUN_ONE_BY_ONE;
  bool empty = false;
  for (int j = 0; j < k; ++j) empty = empty || ns[j] == 0;
  if (empty || s->kind != PSG_STORE_SORTED || !sorted_fused() || s->size == 0) {
    PSG_TRY(run_one_by_one(s, k, ops, keys, ns, vals, outs, st));
  } else {
    PSG_TRY(run_sorted(s, k, ops, keys, ns, vals, outs, st, &sv));
  }
  if (k > 1) s->run_last = sv;
  if (served) *served = sv;
  return PSG_OK;
}

int psg_store_set_key_range(psg_store* s, uint64_t key_begin, uint64_t key_end) {
  PSG_REQUIRE(s && s->kind == PSG_STORE_SORTED && key_begin < key_end, PSG_ERR_INVALID,
              "psg_store_set_key_range: a SORTED store and a non-empty range");
  PSG_TRY(drain(s));
  s->key_begin = key_begin;
  s->key_end = key_end;
  return PSG_OK;
}

int psg_store_run_status(psg_store* s, int k, const int* ops, const uint64_t* const* keys, const uint64_t* ns,
                         const void* const* vals, void* const* outs, psg_stream stream, int* served, int* status) {
  PSG_REQUIRE(s && status && k >= 1 && k <= kMaxFrames, PSG_ERR_INVALID, "psg_store_run_status: bad arguments");
  for (int j = 0; j < k; ++j) status[j] = PSG_OK;
  s->run_status = status;
  const int rc = psg_store_run(s, k, ops, keys, ns, vals, outs, stream, served);
  s->run_status = nullptr;
  if (rc != PSG_OK) {
    // a failure one_status did not record (an argument check, a launch of a
    // one-pass form) applied nothing: every request carries it
    bool recorded = false;
    for (int j = 0; j < k; ++j) recorded = recorded || status[j] != PSG_OK;
    if (!recorded)
      for (int j = 0; j < k; ++j) status[j] = rc;
  }
  return rc;
}

int psg_store_push_slots_frames(psg_store* s, const uint32_t* slots, uint64_t first, const void* const* vals_host,
                                int k, uint64_t n, psg_stream stream) {
  PSG_TRY(frames_args(s, vals_host, k));
  if (n == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(drain(s));
  if (!slots) {
    const uint64_t limit = s->kind == PSG_STORE_SORTED ? s->size : s->capacity;
    PSG_REQUIRE(first <= limit && n <= limit - first, PSG_ERR_RANGE,
                "push frames: slots [%llu, %llu) past the store's %llu", (unsigned long long)first,
                (unsigned long long)(first + n), (unsigned long long)limit);
    char* at = (char*)s->vals + first * (uint64_t)s->esize;
    if (k == 1 || !frames_on()) {
      for (int j = 0; j < k; ++j) PSG_TRY(dense_request(s->dtype, PSG_PUSH, at, vals_host[j], nullptr, n, st));
      return PSG_OK;
    }
    PSG_TRY(frames_apply(s->dtype, at, limit, vals_host, k, n, nullptr, nullptr, 0, s->flags + F_MISSING, st));
  } else {
    if (k == 1 || !frames_on()) {
      for (int j = 0; j < k; ++j) PSG_TRY(slot_request(s->dtype, PSG_PUSH, s->vals, slots, vals_host[j], nullptr, n, st));
      return PSG_OK;
    }
    PSG_TRY(frames_slots(s->dtype, s->vals, slots, vals_host, k, n, nullptr, 0, s->flags + F_MISSING, st));
  }
  count_run(s, k);
  return PSG_OK;
}

int psg_store_dump(psg_store* s, uint64_t* keys_host, void* vals_host) {
  PSG_REQUIRE(s && vals_host, PSG_ERR_INVALID, "psg_store_dump: null argument");
  PSG_TRY(drain(s));
  PSG_HIP(hipDeviceSynchronize());
  if (s->size == 0) return PSG_OK;
  PSG_HIP(hipMemcpy(vals_host, s->vals, s->size * s->esize, hipMemcpyDeviceToHost));
  if (keys_host) {
    if (s->kind == PSG_STORE_SORTED) {
      PSG_HIP(hipMemcpy(keys_host, s->keys, s->size * sizeof(uint64_t), hipMemcpyDeviceToHost));
    } else {
      for (uint64_t i = 0; i < s->size; ++i) keys_host[i] = s->key_begin + i;
    }
  }
  return PSG_OK;
}

}  // extern "C"
