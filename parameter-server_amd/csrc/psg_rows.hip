// psg_rows.hip — the row-valued HBM table (psg_table_*): arbitrary uint64 keys,
// each holding a row of `width` elements of one dtype.
//
// Reference: the same server loop as the scalar store, KVServerDefaultHandle
// (src/ps/KVApp.h:446-454), applied to the k = vals.size() / keys.size() values
// a worker slices per key (DefaultSlicer, src/ps/KVApp.h:515-574):
//     for j < width:  row(key_i)[j] += vals[i * width + j];
//                     out[i * width + j] = row(key_i)[j];
//
// Layout: a sorted key array K[S] and the rows in the same order in one array
// R[S x width]; growth x2; an insert is a merge into new arrays that moves
// whole rows (the width-wide analogue of psg_store.hip's merge_insert).
//
// A request is two passes with the host between them:
//   k_rows_resolve   reads each key once: strict ascent against its
//                    predecessor, the range, its place in K (a search inside
//                    the stretch of K its 1024-key tile spans) -> a uint32 slot
//                    (UINT32_MAX: absent) and the request flags.  The host
//                    reads the flags (one synchronisation), rejects the request
//                    before anything was written, or inserts the absent keys
//                    (compact_count / compact_emit, psg_internal.h) and
//                    resolves again.
//   k_rows_walk      the rows: lanes run over a tile's rows as one flat stream
//                    of 16-B vectors (rows of a multiple of 16 B) or of single
//                    elements, so consecutive slots read and write consecutive
//                    memory; one writer per row (keys are unique): no atomics.
//                    What is done to a row is the walk's unit type: AccUnit
//                    (row += vals) or OptUnit (the optimizer update).
// Algorithmic bytes per f32 key of a Push: key 8 + slot 4 + 4 + 12 * width.
// A list that is not strictly ascending (psg_table_*_any) is sorted, cut into
// its unique keys and their occurrences (plan_any) and served by
// k_rows_walk_seg, the same units over each unique row's occurrences.
// serve() is the body of all four request calls.
//
// The optimizer update (psg_table_update) is the same two passes on OptUnit:
// the async-mode LRServer handle (tests/src/LRServer.h:179-189) with SGD or
// Adam (tests/src/Adam.h:28-34) on the rows a gradient Push names.  The Adam
// moments are f64 rows beside the value rows, one array M[S x 2 width] in slot
// order: a row's m values, then
// its v values, so one row's state is one contiguous run and an insert moves
// it with one k_rows_move of `width` 16-B units through the same slot map.
// Where width is a multiple of 4 each half is kept in the lane order of the
// 16-B path (mom_col below).
//
// The merged update (psg_table_update_merged) is the sync-mode round
// (LRServer.h:151-178) on rows: k gradient frames summed per key from zero in
// arrival order, then one OptUnit::step per key.  Frames that all carry one
// ascending list are served by k_rows_walk_same behind the strict front half;
// anything else by the plan of the concatenated lists and k_rows_walk_merge.
//
// Assign and export (psg_table_assign / psg_table_export) are the two halves of
// a saved model (LRServer.h:36-63, 107-115).  Assign is a strict request on
// SetUnit, which stores the request's row as bytes and never reads the old one;
// export copies a stretch of K and R, which are in key order already.  The
// moments go through k_mom_move in either direction, between the mom_col layout
// and plain column order.
//
// Lookup and erase (psg_table_lookup / psg_table_erase) are the two calls that
// never insert: the reference's store[key] inserts on every access and never
// erases (KVApp.h:446-454), which an evaluation pass or a table over a stream of
// ids cannot live with.  Both resolve a list in any order without sorting it
// (k_rows_resolve_any).  A lookup then reads on ReadUnit behind a flag on the
// device (k_rows_read): two kernels, one synchronisation.  An erase marks the
// named slots, compacts the survivors in order and gathers keys, rows and
// moment rows into new arrays (k_rows_take): insert_missing backwards.
//
// The pooled calls (psg_table_lookup_pooled / psg_table_update_pooled) serve a
// sparse feature as its model consumes it: ids in bags (offsets[nb + 1]), one
// row per BAG across the interface.  The reference has no pooling; the forward
// is the lookup's two kernels with k_rows_pool in k_rows_read's place (a lane
// sums its unit of a bag's rows in arrival order and stores once), the backward
// is the merged round's front half on one list with the bag's gradient row in
// every occurrence's place (k_bag_of, k_rows_walk_pool).  k_offsets_check runs
// in front of either, and nothing walks an offsets array it refused.
//
// The round of pooled and plain frames (psg_table_update_pooled_merged) is the
// merged round's sorted path with the pooled update's payload: the k key lists
// sorted as one with, per occurrence, the index of its gradient row in the
// frames' gradient arrays laid end to end (k_bag_of / k_row_index from each
// frame's first row), and k_rows_walk_pool picking the frame's array with
// frame_of, as k_rows_walk_merge does.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "psg_internal.h"

struct psg_table {
  int dtype;
  int esize;
  uint32_t width;
  uint64_t key_begin, key_end;
  uint64_t size;      // rows present
  uint64_t capacity;  // rows allocated
  void* rows;         // device, capacity * width * esize
  uint64_t* keys;     // device, capacity
  uint32_t* slots;    // device scratch: the request's slots
  uint64_t slots_cap;
  int* flags;       // device view of flags_host
  int* flags_host;  // pinned host int[kNFlags], raised by k_rows_resolve
  // Adam state (psg_table_set_adam): the parameters of Adam.h:14-18 and the
  // moments, capacity * 2 * width doubles in slot order (null while capacity == 0)
  int adam;
  double alr, beta1, beta2, eps;
  double* mom;
  // scratch of the order-preserving requests (psg_table_*_any): the sort's
  // buffers, perm, U and seg carved from one block grown on demand
  void* any_buf;
  uint64_t any_bytes;
  // psg_table_lookup's flag words on the device (kNFlags ints, on first use):
  // raised by its resolve and read by its walk, with no host in between
  int* gate;
  // what a new row starts from (psg_table_set_init): PSG_INIT_ZERO until it is
  // set, then the triple of PSG_INIT_UNIFORM; init_set: the one call was made
  int init_kind, init_set;
  uint64_t init_seed;
  float init_lo, init_hi;
};

namespace psg {
namespace {

constexpr int kRowTile = 1024;  // request keys per block of the resolve (4 per lane)
constexpr uint32_t kAbsent = 0xffffffffu;
constexpr uint64_t kMaxRows = 0xfffffffeull;

// R_DIFFER: raised by k_keys_differ (psg_table_update_merged), after the resolve;
// R_OFFSETS: raised by k_offsets_check (the pooled calls), in front of it
enum { R_MISSING = 0, R_RANGE = 1, R_UNSORTED = 2, R_DIFFER = 3, R_OFFSETS = 4, kNFlags = 5 };

__device__ __forceinline__ void raise(int* flags, int which, bool cond) {
  if (__ballot(cond) && (threadIdx.x & 63) == 0) flags[which] = 1;
}

// Pass 1.  Tile = 1024 request keys; waves 0 and 1 bracket the tile's keys in
// K (lower_bound_wave of its first and last key), every lane then searches only
// that stretch: ~10 steps over lines its neighbours share when the request
// covers a stretch of the table.  A list out of order gives a meaningless (but
// in-bounds) bracket; its request is rejected by the flags.
__global__ __launch_bounds__(256) void k_rows_resolve(const uint64_t* __restrict__ q, uint64_t n,
                                                      const uint64_t* __restrict__ K, uint64_t S, uint64_t kb,
                                                      uint64_t ke, uint32_t* __restrict__ slots,
                                                      int* __restrict__ flags) {
  __shared__ uint64_t win[2];
  const uint64_t ntiles = (n + kRowTile - 1) / kRowTile;
  int missing = 0, range = 0, unsorted = 0;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * kRowTile;
    const uint64_t t1 = t0 + kRowTile < n ? t0 + kRowTile : n;
    const int w = threadIdx.x >> 6;
    if (w == 0) {
      const uint64_t lo = lower_bound_wave(K, S, q[t0]);
      if ((threadIdx.x & 63) == 0) win[0] = lo;
    } else if (w == 1) {
      uint64_t hi = lower_bound_wave(K, S, q[t1 - 1]);
      hi = hi < S ? hi + 1 : S;
      if ((threadIdx.x & 63) == 0) win[1] = hi;
    }
    __syncthreads();
    const uint64_t lo = win[0];
    const uint64_t hi = win[1] > lo ? win[1] : lo;
#pragma unroll
    for (int k = 0; k < kRowTile / kBlock; ++k) {
      const uint64_t i = t0 + (uint64_t)k * kBlock + threadIdx.x;
      if (i >= t1) continue;
      const uint64_t key = q[i];
      if (i > 0 && q[i - 1] >= key) unsorted = 1;
      if (key < kb || key >= ke) range = 1;
      const uint64_t p = lower_bound_dev(K, lo, hi, key);
      const bool found = p < S && K[p] == key;
      if (!found) missing = 1;
      slots[i] = found ? (uint32_t)p : kAbsent;
    }
    __syncthreads();
  }
  raise(flags, R_MISSING, missing != 0);
  raise(flags, R_RANGE, range != 0);
  raise(flags, R_UNSORTED, unsorted != 0);
}

// Pass 1 of the calls that never insert (psg_table_lookup, psg_table_erase):
// the same tile and the same search for a list in ANY order.  The tile is
// bracketed by its smallest and largest key (a wave reduction, then four words
// of LDS) instead of its first and last, so an ascending list searches the
// stretch k_rows_resolve searches and a shuffled one a wider, still correct
// one.  Order is not looked at: only slots and R_RANGE are written.
__global__ __launch_bounds__(256) void k_rows_resolve_any(const uint64_t* __restrict__ q, uint64_t n,
                                                          const uint64_t* __restrict__ K, uint64_t S, uint64_t kb,
                                                          uint64_t ke, uint32_t* __restrict__ slots,
                                                          int* __restrict__ flags) {
  constexpr int PER = kRowTile / kBlock;
  __shared__ uint64_t wmin[kBlock / 64], wmax[kBlock / 64], win[2];
  const uint64_t ntiles = (n + kRowTile - 1) / kRowTile;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int range = 0;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * kRowTile;
    const uint64_t t1 = t0 + kRowTile < n ? t0 + kRowTile : n;
    uint64_t key[PER];
    uint64_t mn = ~0ull, mx = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = t0 + (uint64_t)k * kBlock + threadIdx.x;
      key[k] = i < t1 ? q[i] : 0;
      if (i < t1) {
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
    // lower_bound of the lane's PER keys in K[lo, hi) side by side: the stretch
    // is the block's, so every search takes the same steps, and a step issues
    // the PER probes before it uses one (a shuffled tile spans most of K, and
    // one search at a time is a chain of ~23 dependent loads).  The answer is
    // in [base, base + len]; a probe K[base + half] has base + half < hi <= S.
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
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = t0 + (uint64_t)k * kBlock + threadIdx.x;
      if (i >= t1) continue;
      if (key[k] < kb || key[k] >= ke) range = 1;
      bool found = false;
      uint64_t p = base[k];
      if (len == 1) {  // lower_bound is p, or p + 1 where K[p] < key
        const uint64_t x = K[p];
        found = x == key[k];
        if (x < key[k] && p + 1 < S) found = K[p + 1] == key[k], p = p + 1;
      }
      slots[i] = found ? (uint32_t)p : kAbsent;
    }
    __syncthreads();
  }
  raise(flags, R_RANGE, range != 0);
}

// Merge, keys: old row j goes to j + #(new keys < K[j]), new key t to
// t + #(old keys < M[t]); the places are kept (old_to / new_to) for the rows.
__global__ __launch_bounds__(256) void k_rows_merge_keys(const uint64_t* __restrict__ K, uint64_t S,
                                                         const uint64_t* __restrict__ M, uint64_t m,
                                                         uint64_t* __restrict__ K2, uint32_t* __restrict__ old_to,
                                                         uint32_t* __restrict__ new_to) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < S + m; j += (uint64_t)gridDim.x * kBlock) {
    if (j < S) {
      const uint64_t key = K[j];
      const uint64_t d = j + lower_bound_dev(M, 0, m, key);
      K2[d] = key;
      old_to[j] = (uint32_t)d;
    } else {
      const uint64_t t = j - S;
      const uint64_t key = M[t];
      const uint64_t d = t + lower_bound_dev(K, 0, S, key);
      K2[d] = key;
      new_to[t] = (uint32_t)d;
    }
  }
}

// (RowWalk, a lane's walk over a tile of rows as one flat stream of units, and
// rows_per_tile are in psg_internal.h: psg_route.hip's kernels walk the same way)

// Merge, rows: dst row to[j] = src row j (src == nullptr: a zero row), for j < nrows.
template <typename U>
__global__ __launch_bounds__(256) void k_rows_move(const U* __restrict__ src, U* __restrict__ dst,
                                                   const uint32_t* __restrict__ to, uint64_t nrows, uint32_t upr,
                                                   uint32_t rpt) {
  const uint64_t ntiles = (nrows + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j0 = t * rpt;
    const uint32_t nr = (uint32_t)(nrows - j0 < rpt ? nrows - j0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t j = j0 + w.r;
      U v = {};
      if (src) v = src[j * upr + w.c];
      dst[(uint64_t)to[j] * upr + w.c] = v;
    }
  }
}

// The move the other way round (psg_table_erase): dst row j = src row from[j],
// for j < nrows.  The writes are consecutive, the reads ascend with gaps.
template <typename U>
__global__ __launch_bounds__(256) void k_rows_take(const U* __restrict__ src, U* __restrict__ dst,
                                                   const uint32_t* __restrict__ from, uint64_t nrows, uint32_t upr,
                                                   uint32_t rpt) {
  const uint64_t ntiles = (nrows + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j0 = t * rpt;
    const uint32_t nr = (uint32_t)(nrows - j0 < rpt ? nrows - j0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += kUnroll * kBlock) {
      U x[kUnroll];
      uint64_t d[kUnroll] = {};
      bool ok[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t j = j0 + w.r;
          x[k] = src[(uint64_t)from[j] * upr + w.c];
          d[k] = j * upr + w.c;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k)
        if (ok[k]) dst[d[k]] = x[k];
    }
  }
}

// The slots a list names, marked dead in an array over the table's S slots
// (psg_table_erase); a slot named twice gets the same byte twice.
__global__ __launch_bounds__(256) void k_mark_dead(const uint32_t* __restrict__ slots, uint64_t n,
                                                   uint8_t* __restrict__ dead) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t s = slots[i];
    if (s != kAbsent) dead[s] = 1;
  }
}

template <int DT, bool VEC> struct Unit;
template <int DT> struct Unit<DT, true> {
  typedef u32x4 U;
  __device__ static inline U add(U a, U b) { return Elem<DT>::add(a, b); }
};
template <int DT> struct Unit<DT, false> {
  typedef typename Elem<DT>::T U;
  __device__ static inline U add(U a, U b) { return Elem<DT>::add1(a, b); }
};

// ---- the row units --------------------------------------------------------------
// What a lane holds of one row while it serves it.  A unit is a 16-B vector
// (VEC) or one element, column c of the row in slot `slot`; R, the request's
// values and its reply are arrays of that type U, so every offset counts units.
// The two walks below are written against these members:
//   Params, kDepth  the launch's constants; units a lane of the strict walk
//                   keeps in flight
//   locate          the unit's offsets
//   load_state      the unit of the table's row (and of its moments)
//   load_grad       the unit a request row carries (pushed values or gradients)
//   step            one occurrence applied to the registers
//   store_state     the registers back to the table
//   reply           the registers to a request row's reply

// Accumulate (psg_table_handle): row += vals, per dtype.
template <int DT, bool VEC> struct AccUnit {
  using UT = Unit<DT, VEC>;
  using U = typename UT::U;
  struct Params {};
  static constexpr int kDepth = kUnroll;
  static constexpr bool kPullAlone = true;  // a Pull without a Push is served
  uint64_t so;
  U s;
  __device__ __forceinline__ void locate(uint64_t slot, uint32_t c, uint32_t upr, const Params&) {
    so = slot * upr + c;
  }
  __device__ __forceinline__ void load_state(const U* R, const double*, const Params&) { s = R[so]; }
  __device__ static __forceinline__ U load_grad(const U* vals, uint64_t ro) { return vals[ro]; }
  __device__ __forceinline__ void step(U v, const Params&) { s = UT::add(s, v); }
  __device__ __forceinline__ void store_state(U* R, double*, const Params&) const { R[so] = s; }
  __device__ __forceinline__ void reply(U* out, uint64_t ro) const { out[ro] = s; }
};

// Assign (psg_table_assign): row = the request's row, as bytes.  The unit is an
// unsigned integer of the element's size or a 16-B vector of them, so no value
// ever passes through a floating-point register class: signed zeros, NaN
// payloads, signalling NaNs and subnormals arrive as they were sent.  The old
// row is never read.  Algorithmic bytes per f32 key: key 8 + slot 8 + 8 * width.
template <typename UU> struct SetUnit {
  typedef UU U;
  struct Params {};
  static constexpr int kDepth = kUnroll;
  uint64_t so;
  U s;
  __device__ __forceinline__ void locate(uint64_t slot, uint32_t c, uint32_t upr, const Params&) {
    so = slot * upr + c;
  }
  __device__ __forceinline__ void load_state(const U*, const double*, const Params&) {}
  __device__ static __forceinline__ U load_grad(const U* vals, uint64_t ro) { return vals[ro]; }
  __device__ __forceinline__ void step(U v, const Params&) { s = v; }
  __device__ __forceinline__ void store_state(U* R, double*, const Params&) const { R[so] = s; }
  __device__ __forceinline__ void reply(U* out, uint64_t ro) const { out[ro] = s; }
};

// Read (psg_table_lookup): the reply is the row as bytes, and a key the table
// does not hold (slot kAbsent) answers with a zero row that is never loaded.
// The unit is SetUnit's: an unsigned integer of the element's size or a 16-B
// vector of them.  Nothing is stored to the table, so the unit has no step.
// Algorithmic bytes per f32 key: key 8 + slot 8 + 8 * width (+ 1 for found).
template <typename UU> struct ReadUnit {
  typedef UU U;
  static constexpr int kDepth = kUnroll;
  uint64_t so;
  bool present;
  U s;
  __device__ __forceinline__ void locate(uint32_t slot, uint32_t c, uint32_t upr) {
    present = slot != kAbsent;
    so = present ? (uint64_t)slot * upr + c : 0;
  }
  __device__ __forceinline__ void load_state(const U* R) {
    s = U{};
    if (present) s = R[so];
  }
  __device__ __forceinline__ void reply(U* out, uint64_t ro) const { out[ro] = s; }
};

// Pool (psg_table_lookup_pooled): what a lane keeps of one bag while it sums it.
// U is the unit as the table stores it (a 16-B vector, or one element), A the
// running sum: f32 for F32 / F16 / BF16 rows, f64 for F64 rows, one lane of A per
// element of the unit (PoolAcc, psg_internal.h, which psg_pool_reduce shares).

// ---- the optimizer update ----------------------------------------------------
// Where in its half (m or v) of a moment row the moment of column j lives.
// width % 4 == 0: the unit of four columns 4u..4u+3 keeps the pair (4u, 4u+1)
// at doubles 2u, 2u+1 and the pair (4u+2, 4u+3) at width/2 + 2u, so a lane of
// the 16-B path, which owns one unit, loads each pair as 16 B and consecutive
// lanes load consecutive memory: four runs of 16 B a lane per wave instruction
// instead of two 32-B-strided ones that each touch half of every line (what
// psg_lr.hip's QUAD layout does for the dense weights).  Other widths: column
// order.
__host__ __device__ inline uint32_t mom_col(uint32_t j, uint32_t width) {
  if (width % 4) return j;
  return ((j >> 1) & 1) * (width / 2) + 2 * (j >> 2) + (j & 1);
}

struct AdamArgs {
  double alr, b1, b2, eps, c1, c2;
};

// Optimize (psg_table_update), F32 rows.  Per element (LRServer.h:182-189,
// Adam.h:28-34):
//   g = (double)(lr * grad); Adam: m, v updated, g = alr * (m / c1) / (sqrt(v / c2) + eps);
//   row = (float)((double)row - g); the Pull's reply is the updated row.
// VEC: a unit is four columns (16 B of gradient, 16 B of row, four 16-B moment
// pairs in the mom_col layout); else one column.  SGD keeps kUnroll units in
// flight, Adam two (24 data registers a unit and the f64 divide and square
// root on top).  This is the one copy of the arithmetic: it matches the
// reference bit for bit, in this operation order and without contraction.
template <bool ADAM, bool VEC> struct OptUnit {
  static constexpr int E = VEC ? 4 : 1;
  typedef typename std::conditional<VEC, f32x4, float>::type U;
  struct Params {
    uint32_t width;
    float lr;
    AdamArgs a;
  };
  static constexpr int kDepth = ADAM ? 2 : kUnroll;
  static constexpr bool kPullAlone = false;
  float s[E];
  double q[2 * E];  // m of the unit's columns, then v
  uint64_t so, mo;  // offsets of the unit: row (units), m (doubles)
  __device__ __forceinline__ void locate(uint64_t slot, uint32_t c, uint32_t upr, const Params& p) {
    so = slot * upr + c;
    if constexpr (ADAM) mo = slot * 2 * p.width + (VEC ? 2 * c : mom_col(c, p.width));
  }
  __device__ __forceinline__ void load_state(const U* R, const double* M, const Params& p) {
    if constexpr (VEC) {
      const f32x4 sv = R[so];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = sv[e];
      if constexpr (ADAM) {
        const uint32_t half = p.width / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f64x2 pr = *reinterpret_cast<const f64x2*>(M + mo + (uint64_t)r * half);
          q[2 * r] = pr[0], q[2 * r + 1] = pr[1];
        }
      }
    } else {
      s[0] = R[so];
      if constexpr (ADAM) q[0] = M[mo], q[1] = M[mo + p.width];
    }
  }
  __device__ static __forceinline__ U load_grad(const U* grads, uint64_t ro) { return grads[ro]; }
  __device__ __forceinline__ void step(U gu, const Params& p) {
    const float lr = p.lr;
    const AdamArgs& a = p.a;
    float g[E];
    if constexpr (VEC) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = gu[e];
    } else {
      g[0] = gu;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double gr = (double)(lr * g[e]);
      if constexpr (ADAM) {
        const double mi = a.b1 * q[e] + (1.0 - a.b1) * gr;
        const double vi = a.b2 * q[E + e] + (1.0 - a.b2) * gr * gr;
        q[e] = mi;
        q[E + e] = vi;
        gr = a.alr * (mi / a.c1) / (sqrt(vi / a.c2) + a.eps);
      }
      s[e] = (float)((double)s[e] - gr);
    }
  }
  __device__ __forceinline__ U packed() const {
    if constexpr (VEC) return f32x4{s[0], s[1], s[2], s[3]};
    else return s[0];
  }
  __device__ __forceinline__ void store_state(U* R, double* M, const Params& p) const {
    if constexpr (ADAM) {
      if constexpr (VEC) {
        const uint32_t half = p.width / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<f64x2*>(M + mo + (uint64_t)r * half) = f64x2{q[2 * r], q[2 * r + 1]};
      } else {
        M[mo] = q[0], M[mo + p.width] = q[1];
      }
    }
    R[so] = packed();
  }
  __device__ __forceinline__ void reply(U* out, uint64_t ro) const { out[ro] = packed(); }
};

// ---- the two walks --------------------------------------------------------------
// Pass 2 of the strict calls.  Request row i (slot slots[i]) for i < n; every
// slot is present.  Lanes run over a tile's rows as one flat stream of units,
// kDepth of them in flight: every load of a step is issued before its
// arithmetic.  One writer per row (keys are unique): no atomics.
template <typename UNIT, int OP>
__global__ __launch_bounds__(256) void k_rows_walk(typename UNIT::U* __restrict__ R, double* __restrict__ M,
                                                   const uint32_t* __restrict__ slots,
                                                   const typename UNIT::U* __restrict__ vals,
                                                   typename UNIT::U* __restrict__ out, uint64_t n, uint32_t upr,
                                                   uint32_t rpt, typename UNIT::Params prm) {
  constexpr int UN = UNIT::kDepth;
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UN * kBlock) {
      // u and ro start from zero: left unset, a unit past the tile's end would
      // carry the last step's registers around the loop (6 more VGPRs for Adam)
      UNIT u[UN] = {};
      typename UNIT::U g[UN];
      uint64_t ro[UN] = {};  // the unit's offset in the request
      bool ok[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t i = i0 + w.r;
          u[k].locate(slots[i], w.c, upr, prm);
          ro[k] = i * upr + w.c;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!ok[k]) continue;
        u[k].load_state(R, M, prm);
        if constexpr ((OP & PSG_PUSH) != 0) g[k] = UNIT::load_grad(vals, ro[k]);
      }
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!ok[k]) continue;
        if constexpr ((OP & PSG_PUSH) != 0) {
          u[k].step(g[k], prm);
          u[k].store_state(R, M, prm);
        }
        if constexpr ((OP & PSG_PULL) != 0) u[k].reply(out, ro[k]);
      }
    }
  }
}

// Pass 2 of psg_table_lookup: k_rows_walk's flat stream over the request's n
// rows on ReadUnit, launched behind k_rows_resolve_any WITHOUT the host in
// between.  What the host would have checked is checked here: `gate` is the
// device word the resolve raised R_RANGE in, and a launch that finds it set
// writes nothing.  An absent slot is allowed and loads nothing.  found[i] is
// written by the lane that holds column 0 of row i: once per row.  out null:
// presence only, one lane per row.
template <typename U>
__global__ __launch_bounds__(256) void k_rows_read(const U* __restrict__ R, const uint32_t* __restrict__ slots,
                                                   U* __restrict__ out, uint8_t* __restrict__ found, uint64_t n,
                                                   uint32_t upr, uint32_t rpt, const int* __restrict__ gate) {
  using UNIT = ReadUnit<U>;
  constexpr int UN = UNIT::kDepth;
  if (gate[R_RANGE]) return;
  if (!out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
      found[i] = slots[i] != kAbsent ? 1 : 0;
    return;
  }
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UN * kBlock) {
      UNIT u[UN] = {};
      uint64_t ro[UN] = {};  // the unit's offset in the reply
      bool ok[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t i = i0 + w.r;
          u[k].locate(slots[i], w.c, upr);
          ro[k] = i * upr + w.c;
          if (found && w.c == 0) found[i] = u[k].present ? 1 : 0;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) u[k].load_state(R);
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) u[k].reply(out, ro[k]);
    }
  }
}

// ---- the pooled lookup (psg_table_lookup_pooled) -----------------------------------
// The three rules of a bag list, over its nb + 1 words: offsets[0] == 0, no
// offset above its successor, offsets[nb] == n.  Together they put every bag
// inside [0, n).  8 B read per bag; it runs in front of everything else that
// reads `offsets`, and a kernel behind it that finds R_OFFSETS raised walks nothing.
__global__ __launch_bounds__(256) void k_offsets_check(const uint64_t* __restrict__ offsets, uint64_t nb, uint64_t n,
                                                       int* __restrict__ flags) {
  int bad = 0;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * kBlock) {
    const uint64_t o = offsets[b];
    if (b == 0 && o != 0) bad = 1;
    if (b == nb ? o != n : offsets[b + 1] < o) bad = 1;
  }
  raise(flags, R_OFFSETS, bad != 0);
}

// Pass 2 of psg_table_lookup_pooled, launched behind k_offsets_check and
// k_rows_resolve_any WITHOUT the host in between, as k_rows_read is: `gate` is
// the device word both raised their flags in, and a launch that finds R_RANGE
// or R_OFFSETS set returns before it has read one offset — a refused offsets
// array would send the walk out of `slots`.  Lanes take (bag, unit) pairs as
// k_rows_walk_seg takes (unique row, unit) pairs.  A lane walks its bag's slots
// in arrival order, adds its unit of every present row to a sum that starts
// from +0 (ACC: PoolAcc) and stores once: one writer per unit of the reply, no
// atomics, no LDS.  The loop is a chain slots -> row unit -> add; the slot two
// ahead and the row unit one ahead are loaded before the current add.  An
// absent slot (kAbsent) loads nothing and adds nothing.
// POOL (psg_table_lookup_pooled_weighted): kPoolWeighted reads weights[p] beside
// slots[p], two ahead as the slot is, and adds ACC::times(weight, unit) — one
// multiply, then sum's one add; the chain is slots, weights -> row unit -> mul ->
// add.  An absent slot's weight is loaded and not used.  kPoolMean divides the
// sum of a bag that holds a position by its length (ACC::over) before the one
// store.  kPoolSum reads no weight and is the code it was.
enum { kPoolSum = 0, kPoolWeighted = 1, kPoolMean = 2 };
template <typename U, typename ACC, int POOL = kPoolSum>
__global__ __launch_bounds__(256) void k_rows_pool(const U* __restrict__ R, const uint32_t* __restrict__ slots,
                                                   const uint64_t* __restrict__ offsets, U* __restrict__ out,
                                                   uint64_t nb, uint32_t upr, uint32_t rpt,
                                                   const int* __restrict__ gate,
                                                   const float* __restrict__ weights = nullptr) {
  if (gate[R_RANGE] | gate[R_OFFSETS]) return;
  const uint64_t ntiles = (nb + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t b0 = t * rpt;
    const uint32_t nr = (uint32_t)(nb - b0 < rpt ? nb - b0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t b = b0 + w.r;
      const uint32_t c = w.c;
      uint32_t p = (uint32_t)offsets[b];  // <= n <= 2^32 - 2: checked
      const uint32_t pe = (uint32_t)offsets[b + 1];
      [[maybe_unused]] const uint32_t len = pe - p;
      typename ACC::A acc = {};  // +0
      if (p < pe) {
        uint32_t s0 = slots[p];
        uint32_t s1 = p + 1 < pe ? slots[p + 1] : kAbsent;
        [[maybe_unused]] float w0 = 0, w1 = 0;
        if constexpr (POOL == kPoolWeighted) {
          w0 = weights[p];
          if (p + 1 < pe) w1 = weights[p + 1];
        }
        U v = {};
        if (s0 != kAbsent) v = R[(uint64_t)s0 * upr + c];
        for (; p < pe; ++p) {
          const uint32_t s2 = p + 2 < pe ? slots[p + 2] : kAbsent;
          [[maybe_unused]] float w2 = 0;
          if constexpr (POOL == kPoolWeighted)
            if (p + 2 < pe) w2 = weights[p + 2];
          U vn = {};
          if (s1 != kAbsent) vn = R[(uint64_t)s1 * upr + c];
          if constexpr (POOL == kPoolWeighted) {
            if (s0 != kAbsent) acc = ACC::sum(acc, ACC::times(w0, v));
            w0 = w1, w1 = w2;
          } else {
            if (s0 != kAbsent) acc = ACC::add(acc, v);
          }
          s0 = s1, s1 = s2, v = vn;
        }
        if constexpr (POOL == kPoolMean) acc = ACC::over(acc, len);
      }
      out[b * upr + c] = ACC::round(acc);
    }
  }
}

// ---- the initial rows (psg_table_set_init / psg_init_rows) ------------------------
// Element j of the initial row of key K (include/psg.h): word j % 4 of
// Philox4x32-10 on the counter {K lo, K hi, j / 4, 0} under the key {seed lo,
// seed hi}; its upper 24 bits as u in [0, 1); lo + u * span in f32, the multiply
// and the add each rounded (the file is built with -ffp-contract=off); then the
// table's dtype.  Nothing else enters, so a row is the same wherever and
// whenever it is made: in the insert's fill, in a lookup that finds its key
// absent, on another server, after a restart.
// A block is ten rounds of two 32 x 32 -> 64 multiplies (20 v_mad_u64_u32).
struct InitSpec {
  uint32_t k0, k1;  // the seed's words
  float lo, span;   // span = hi - lo, subtracted once on the host
};

__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                       uint32_t k1, uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// block b of key's initial row: elements 4b .. 4b + 3 as f32
__device__ __forceinline__ void init_block(uint64_t key, uint32_t b, const InitSpec& s, float v[4]) {
  uint32_t x[4];
  philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), b, 0u, s.k0, s.k1, x);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float u = (float)(x[e] >> 8) * 0x1p-24f;  // exact
    const float prod = u * s.span;
    v[e] = s.lo + prod;
  }
}

// v[w] for a word index that is not a constant: selects, no indexed register file
__device__ __forceinline__ float pick4(const float v[4], uint32_t w) {
  return w == 0 ? v[0] : w == 1 ? v[1] : w == 2 ? v[2] : v[3];
}

// Unit c of key's initial row as the table stores it.  VEC: the 16-B unit (F32:
// one block; F16 / BF16: blocks 2c and 2c + 1, rounded to nearest even; F64:
// half of block c / 2, widened), else element c (its block, one word kept).
template <int DT, bool VEC> struct InitUnit;
template <int DT> struct InitUnit<DT, true> {
  typedef u32x4 U;
  __device__ static __forceinline__ U make(uint64_t key, uint32_t c, const InitSpec& s) {
    float v[8];
    if constexpr (DT == PSG_F32) {
      init_block(key, c, s, v);
      return __builtin_bit_cast(U, f32x4{v[0], v[1], v[2], v[3]});
    } else if constexpr (DT == PSG_F64) {
      init_block(key, c >> 1, s, v);
      const bool up = (c & 1) != 0;
      return __builtin_bit_cast(U, f64x2{(double)(up ? v[2] : v[0]), (double)(up ? v[3] : v[1])});
    } else {
      init_block(key, 2 * c, s, v);
      init_block(key, 2 * c + 1, s, v + 4);
      typename PoolVec<DT>::A a = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
      return __builtin_bit_cast(U, __builtin_convertvector(a, typename PoolVec<DT>::V));
    }
  }
};
template <int DT> struct InitUnit<DT, false> {
  typedef typename Elem<DT>::T T;
  typedef typename std::conditional<sizeof(T) == 8, uint64_t,
                                    typename std::conditional<sizeof(T) == 4, uint32_t, uint16_t>::type>::type U;
  __device__ static __forceinline__ U bits(float x) { return __builtin_bit_cast(U, (T)x); }
  __device__ static __forceinline__ U make(uint64_t key, uint32_t c, const InitSpec& s) {
    float v[4];
    init_block(key, c >> 2, s, v);
    return bits(pick4(v, c & 3));
  }
};

// The initial rows of keys[j] for j < nrows: row j of dst, or row to[j] where
// `to` is not null (insert_missing: miss and new_to).  VEC: a lane makes and
// stores one 16-B unit.  Else a lane makes ONE block and stores its up to four
// elements (the row's last block may be short); upr counts blocks, (width + 3) /
// 4.  Consecutive lanes write consecutive memory either way; one writer per
// element.  Per 16 B written: 20 wide multiplies (F32), 40 (halves), 10 (F64).
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void k_rows_init(typename InitUnit<DT, VEC>::U* __restrict__ dst,
                                                   const uint64_t* __restrict__ keys, const uint32_t* __restrict__ to,
                                                   uint64_t nrows, uint32_t width, uint32_t upr, uint32_t rpt,
                                                   InitSpec spec) {
  const uint64_t ntiles = (nrows + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j0 = t * rpt;
    const uint32_t nr = (uint32_t)(nrows - j0 < rpt ? nrows - j0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t j = j0 + w.r;
      const uint64_t key = keys[j];
      const uint64_t row = to ? (uint64_t)to[j] : j;
      if constexpr (VEC) {
        dst[row * upr + w.c] = InitUnit<DT, true>::make(key, w.c, spec);
      } else {
        float v[4];
        init_block(key, w.c, spec, v);
        const uint32_t c0 = 4 * w.c;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < width) dst[row * width + c0 + k] = InitUnit<DT, false>::bits(v[k]);
      }
    }
  }
}

// k_rows_read for a table with an initializer: the same walk, and a unit whose
// slot is kAbsent is made from its key (q[i], loaded by absent lanes only) in
// the place where k_rows_read leaves zeros — the bytes an insert would store.
// found[i] is still 0.  The present rows' loads are issued as they were, before
// the first block is computed.  VEC: 16-B units; else single elements, each
// absent element computing its own block (a lookup's absent ids are the
// exception; the insert's fill is the path that shares a block).
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void k_rows_read_init(const typename InitUnit<DT, VEC>::U* __restrict__ R,
                                                        const uint32_t* __restrict__ slots,
                                                        const uint64_t* __restrict__ q,
                                                        typename InitUnit<DT, VEC>::U* __restrict__ out,
                                                        uint8_t* __restrict__ found, uint64_t n, uint32_t upr,
                                                        uint32_t rpt, const int* __restrict__ gate, InitSpec spec) {
  using U = typename InitUnit<DT, VEC>::U;
  using UNIT = ReadUnit<U>;
  constexpr int UN = UNIT::kDepth;
  if (gate[R_RANGE]) return;
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UN * kBlock) {
      UNIT u[UN] = {};
      uint64_t ro[UN] = {};  // the unit's offset in the reply
      uint64_t key[UN] = {};
      uint32_t col[UN] = {};
      bool ok[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t i = i0 + w.r;
          u[k].locate(slots[i], w.c, upr);
          ro[k] = i * upr + w.c;
          col[k] = w.c;
          if (!u[k].present) key[k] = q[i];
          if (found && w.c == 0) found[i] = u[k].present ? 1 : 0;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) u[k].load_state(R);
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!ok[k]) continue;
        if (!u[k].present) u[k].s = InitUnit<DT, VEC>::make(key[k], col[k], spec);
        u[k].reply(out, ro[k]);
      }
    }
  }
}

// k_rows_pool for a table with an initializer: the same chain (slot two ahead,
// row unit one ahead), and the unit "one ahead" of an absent slot is made from
// its key where k_rows_pool loads nothing; every position of the bag then adds
// (times its weight, for kPoolWeighted), so a pooled lookup is the sum the
// model will see once the update has inserted the id.  Only absent lanes load a
// key and compute blocks.
template <int DT, bool VEC, int POOL>
__global__ __launch_bounds__(256) void k_rows_pool_init(const typename PoolAcc<DT, VEC>::U* __restrict__ R,
                                                        const uint32_t* __restrict__ slots,
                                                        const uint64_t* __restrict__ q,
                                                        const uint64_t* __restrict__ offsets,
                                                        typename PoolAcc<DT, VEC>::U* __restrict__ out, uint64_t nb,
                                                        uint32_t upr, uint32_t rpt, const int* __restrict__ gate,
                                                        const float* __restrict__ weights, InitSpec spec) {
  using ACC = PoolAcc<DT, VEC>;
  using U = typename ACC::U;
  using INIT = InitUnit<DT, VEC>;
  static_assert(sizeof(U) == sizeof(typename INIT::U), "one unit size");
  if (gate[R_RANGE] | gate[R_OFFSETS]) return;
  const uint64_t ntiles = (nb + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t b0 = t * rpt;
    const uint32_t nr = (uint32_t)(nb - b0 < rpt ? nb - b0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t b = b0 + w.r;
      const uint32_t c = w.c;
      uint32_t p = (uint32_t)offsets[b];  // <= n <= 2^32 - 2: checked
      const uint32_t pe = (uint32_t)offsets[b + 1];
      [[maybe_unused]] const uint32_t len = pe - p;
      auto unit_at = [&](uint32_t slot, uint32_t pos) -> U {
        if (slot != kAbsent) return R[(uint64_t)slot * upr + c];
        return __builtin_bit_cast(U, INIT::make(q[pos], c, spec));
      };
      typename ACC::A acc = {};  // +0
      if (p < pe) {
        uint32_t s1 = p + 1 < pe ? slots[p + 1] : kAbsent;
        [[maybe_unused]] float w0 = 0, w1 = 0;
        if constexpr (POOL == kPoolWeighted) {
          w0 = weights[p];
          if (p + 1 < pe) w1 = weights[p + 1];
        }
        U v = unit_at(slots[p], p);
        for (; p < pe; ++p) {
          const uint32_t s2 = p + 2 < pe ? slots[p + 2] : kAbsent;
          [[maybe_unused]] float w2 = 0;
          if constexpr (POOL == kPoolWeighted)
            if (p + 2 < pe) w2 = weights[p + 2];
          U vn = {};
          if (p + 1 < pe) vn = unit_at(s1, p + 1);
          if constexpr (POOL == kPoolWeighted) {
            acc = ACC::sum(acc, ACC::times(w0, v));
            w0 = w1, w1 = w2;
          } else {
            acc = ACC::add(acc, v);
          }
          s1 = s2, v = vn;
        }
        if constexpr (POOL == kPoolMean) acc = ACC::over(acc, len);
      }
      out[b * upr + c] = ACC::round(acc);
    }
  }
}

// ---- the moments in and out (psg_table_assign / psg_table_export) ---------------
// Request row i (slot slots[i], or first + i where slots is null) for i < n:
// its moments between the table's moment row (mom_col layout) and the plain
// arrays m, v of n * width doubles in column order.  TO_TABLE: plain -> table,
// else table -> plain.  A unit is U: a pair of doubles (width % 4 == 0 and
// m, v on 16 B) or one double; a moment row is 2 * width / E units, its m half
// first.  Unit p of a half holds columns p * E .. and lives at mom_col(p * E):
// mom_col keeps a pair of columns (2p, 2p + 1) together, so pairs of lanes
// move 32 consecutive bytes on both sides.  kUnroll units in flight, every load
// before the first store; one writer per unit, no atomics.
template <typename U, bool TO_TABLE>
__global__ __launch_bounds__(256) void k_mom_move(double* __restrict__ M, const uint32_t* __restrict__ slots,
                                                  uint64_t first, double* __restrict__ m, double* __restrict__ v,
                                                  uint64_t n, uint32_t width, uint32_t rpt) {
  constexpr uint32_t E = sizeof(U) / sizeof(double);
  const uint32_t uph = width / E;  // units per half
  const uint32_t upr = 2 * uph;
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += kUnroll * kBlock) {
      U x[kUnroll];
      U* dst[kUnroll] = {};
      bool ok[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t i = i0 + w.r;
          const uint64_t slot = slots ? (uint64_t)slots[i] : first + i;
          const uint32_t h = w.c >= uph ? 1u : 0u;
          const uint32_t j = (w.c - h * uph) * E;  // the unit's first column
          U* tab = reinterpret_cast<U*>(M + slot * 2 * width + h * width + mom_col(j, width));
          U* pln = reinterpret_cast<U*>((h ? v : m) + i * width + j);
          x[k] = *(TO_TABLE ? pln : tab);
          dst[k] = TO_TABLE ? tab : pln;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k)
        if (ok[k]) *dst[k] = x[k];
    }
  }
}

// ---- the order-preserving request (psg_table_*_any) ---------------------------
// The list is sorted stably by key with its positions (radix_sort_u64, iota):
// sorted[n] and perm[n].  The heads of the runs of equal keys (RunHead) give
// the strictly ascending unique list U[m] and seg[m + 1], the bounds of each
// key's occurrences in perm — in arrival order, the sort being stable.
struct EmitHead {
  const uint64_t* sorted;
  uint64_t n;
  uint64_t* U;
  uint32_t* seg;
  __device__ void operator()(uint64_t i, uint32_t pos) const {
    U[pos] = sorted[i];
    seg[pos] = (uint32_t)i;
  }
  __device__ void done(uint32_t m) const { seg[m] = (uint32_t)n; }
};

// The survivors of an erase, in slot (= key) order: their keys and old slots.
struct Alive {
  const uint8_t* dead;
  __device__ bool operator()(uint64_t i) const { return dead[i] == 0; }
};
struct EmitSurvivor {
  const uint64_t* K;
  uint64_t* K2;
  uint32_t* from;
  __device__ void operator()(uint64_t i, uint32_t pos) const {
    K2[pos] = K[i];
    from[pos] = (uint32_t)i;
  }
  __device__ void done(uint32_t) const {}
};

// Pass 2 of the any-order calls.  Unique row u (slot slots[u]) for u < m; its
// occurrences are request rows perm[seg[u] .. seg[u + 1]), in arrival order.
// The lanes walk the unique rows as k_rows_walk walks request rows; a lane
// loads its unit of the row (and its moments) once, runs over the occurrences
// (step, reply with the running row) and stores the unit once: one writer per
// row, no atomics.  The loop is a chain perm -> vals -> step; the position two
// ahead and the values one ahead are loaded before the current step.
template <typename UNIT, int OP>
__global__ __launch_bounds__(256) void k_rows_walk_seg(typename UNIT::U* __restrict__ R, double* __restrict__ M,
                                                       const uint32_t* __restrict__ slots,
                                                       const uint32_t* __restrict__ seg,
                                                       const uint32_t* __restrict__ perm,
                                                       const typename UNIT::U* __restrict__ vals,
                                                       typename UNIT::U* __restrict__ out, uint64_t m, uint32_t upr,
                                                       uint32_t rpt, typename UNIT::Params prm) {
  using U = typename UNIT::U;
  const uint64_t ntiles = (m + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t u0 = t * rpt;
    const uint32_t nr = (uint32_t)(m - u0 < rpt ? m - u0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t u = u0 + w.r;
      UNIT x;
      x.locate(slots[u], w.c, upr, prm);
      uint32_t p = seg[u];
      const uint32_t pe = seg[u + 1];  // > p: every unique key has an occurrence
      x.load_state(R, M, prm);
      uint32_t i0 = perm[p];
      uint32_t i1 = p + 1 < pe ? perm[p + 1] : 0;
      U v = {};
      if constexpr ((OP & PSG_PUSH) != 0) v = UNIT::load_grad(vals, (uint64_t)i0 * upr + w.c);
      for (; p < pe; ++p) {
        const uint32_t i2 = p + 2 < pe ? perm[p + 2] : 0;
        U vn = v;
        if constexpr ((OP & PSG_PUSH) != 0) {
          if (p + 1 < pe) vn = UNIT::load_grad(vals, (uint64_t)i1 * upr + w.c);
          x.step(v, prm);
        }
        if constexpr ((OP & PSG_PULL) != 0) x.reply(out, (uint64_t)i0 * upr + w.c);
        i0 = i1, i1 = i2, v = vn;
      }
      if constexpr ((OP & PSG_PUSH) != 0) x.store_state(R, M, prm);
    }
  }
}

// ---- the merged update (psg_table_update_merged) --------------------------------
// k gradient frames, summed per key from +0.0f in arrival order (frame, then
// position), then ONE step per key: the sync-mode round of LRServer.h:151-178 on
// rows.  The frame table goes to the kernels by value.
constexpr int kMaxFrames = 16;
constexpr int kFrameGroup = 4;  // frames whose loads are issued before their ordered adds
struct Frames {
  // k_rows_walk_same: the frames' arrays.  k_rows_walk_merge: each moved back by
  // its frame's off[j] rows, so that a position of the concatenation indexes it
  const void* vals[kMaxFrames];
  void* out[kMaxFrames];
  uint32_t off[kMaxFrames + 1];  // first position of frame j in the concatenation; UINT32_MAX from k on
  int k;
};
struct KeyFrames {
  const uint64_t* p[kMaxFrames];
  int k;
};

// Same-list test over the first n keys: every further key list equals list 0
// element for element (8 B per key per further frame; a frame that IS list 0
// is skipped); with `order`, list 0 also has to ascend strictly there.
__global__ __launch_bounds__(256) void k_keys_differ(KeyFrames f, uint64_t n, int order, int* __restrict__ flags) {
  int differ = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t x = f.p[0][i];
    if (order && i > 0 && f.p[0][i - 1] >= x) differ = 1;
    for (int j = 1; j < f.k; ++j)
      if (f.p[j] != f.p[0] && f.p[j][i] != x) differ = 1;
  }
  raise(flags, R_DIFFER, differ != 0);
}

// Pass 2 of the same-list round: k_rows_walk's flat stream of units over the n
// rows of list 0, every frame carrying its gradients of request row i at row i.
// A unit's gradient is ((0 + f_0[ro]) + f_1[ro]) + ...: the loads of
// kFrameGroup frames are issued before their adds, two units in flight.  Then
// one step, one store, and the reply into every frame's out.
template <typename UNIT, int OP>
__global__ __launch_bounds__(256) void k_rows_walk_same(typename UNIT::U* __restrict__ R, double* __restrict__ M,
                                                        const uint32_t* __restrict__ slots, Frames f, uint64_t n,
                                                        uint32_t upr, uint32_t rpt, typename UNIT::Params prm) {
  using U = typename UNIT::U;
  constexpr int UN = 2;
  const uint64_t ntiles = (n + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * rpt;
    const uint32_t nr = (uint32_t)(n - i0 < rpt ? n - i0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UN * kBlock) {
      UNIT u[UN] = {};
      U s[UN] = {};  // +0.0f: the merge buffer starts from zero
      uint64_t ro[UN] = {};
      bool ok[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        ok[k] = e0 + (uint32_t)k * kBlock < total;
        if (ok[k]) {
          const uint64_t i = i0 + w.r;
          u[k].locate(slots[i], w.c, upr, prm);
          ro[k] = i * upr + w.c;
        }
        w.next();
      }
#pragma unroll
      for (int k = 0; k < UN; ++k)
        if (ok[k]) u[k].load_state(R, M, prm);
      for (int j0 = 0; j0 < f.k; j0 += kFrameGroup) {
        U g[UN][kFrameGroup];
#pragma unroll
        for (int j = 0; j < kFrameGroup; ++j)
#pragma unroll
          for (int k = 0; k < UN; ++k)
            if (j0 + j < f.k && ok[k]) g[k][j] = UNIT::load_grad((const U*)f.vals[j0 + j], ro[k]);
#pragma unroll
        for (int j = 0; j < kFrameGroup; ++j)
#pragma unroll
          for (int k = 0; k < UN; ++k)
            if (j0 + j < f.k && ok[k]) s[k] = s[k] + g[k][j];
      }
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!ok[k]) continue;
        u[k].step(s[k], prm);
        u[k].store_state(R, M, prm);
        if constexpr ((OP & PSG_PULL) != 0)
          for (int j = 0; j < f.k; ++j) u[k].reply((U*)f.out[j], ro[k]);
      }
    }
  }
}

// the frame that holds position pos of the concatenation: the last j with
// off[j] <= pos (an empty frame shares its offset with the next one).  The
// offsets ascend and are the same for every lane (scalar registers), so j is
// the count of off[1 .. 15] <= pos: 15 compares and no load on the lane's
// perm -> gradient chain.
__device__ __forceinline__ uint32_t frame_of(const Frames& f, uint32_t pos) {
  uint32_t j = 0;
#pragma unroll
  for (int i = 1; i < kMaxFrames; ++i) j += f.off[i] <= pos ? 1u : 0u;
  return j;
}

// Pass 2 of the general round.  Unique row u (slot slots[u]) for u < m; its
// occurrences are positions perm[seg[u] .. seg[u + 1]) of the concatenated
// frames, in arrival order (the sort is stable and positions ascend with frame,
// then row).  The lanes walk the unique rows as k_rows_walk_seg does; a lane
// sums its unit over the occurrences from zero (the position two ahead and the
// values one ahead are loaded before the current add), then takes one step on
// the row (and moments) and stores once.  The row's loads are issued in front
// of the loop and used after it: a lane has one unit in flight, so their latency
// runs beside the perm -> gradient chain instead of behind it.  For a Pull it walks the
// segment again and stores the updated unit to every occurrence's reply.  One
// writer per row, no atomics.  A frame's array is picked per lane, so a block
// keeps the (moved-back) array addresses in LDS: one 8-B LDS read an occurrence.
template <typename UNIT, int OP>
__global__ __launch_bounds__(256) void k_rows_walk_merge(typename UNIT::U* __restrict__ R, double* __restrict__ M,
                                                         const uint32_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ seg,
                                                         const uint32_t* __restrict__ perm, Frames f, uint64_t m,
                                                         uint32_t upr, uint32_t rpt, typename UNIT::Params prm) {
  using U = typename UNIT::U;
  __shared__ uint64_t vals_at[kMaxFrames], out_at[kMaxFrames];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < kMaxFrames; ++j) vals_at[j] = (uint64_t)f.vals[j], out_at[j] = (uint64_t)f.out[j];
  }
  __syncthreads();
  const uint64_t ntiles = (m + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t u0 = t * rpt;
    const uint32_t nr = (uint32_t)(m - u0 < rpt ? m - u0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t u = u0 + w.r;
      const uint32_t c = w.c;
      const uint32_t slot = slots[u];
      const uint32_t p0 = seg[u];
      const uint32_t pe = seg[u + 1];  // > p0: every unique key has an occurrence
      auto grad_at = [&](uint32_t pos) {
        return UNIT::load_grad((const U*)vals_at[frame_of(f, pos)], (uint64_t)pos * upr + c);
      };
      UNIT x;
      x.locate(slot, c, upr, prm);
      x.load_state(R, M, prm);  // issued here, used after the sum
      uint32_t i1 = p0 + 1 < pe ? perm[p0 + 1] : 0;
      U v = grad_at(perm[p0]);
      U s = {};  // +0.0f
      for (uint32_t p = p0; p < pe; ++p) {
        const uint32_t i2 = p + 2 < pe ? perm[p + 2] : 0;
        U vn = v;
        if (p + 1 < pe) vn = grad_at(i1);
        s = s + v;
        i1 = i2, v = vn;
      }
      x.step(s, prm);
      x.store_state(R, M, prm);
      if constexpr ((OP & PSG_PULL) != 0) {
        uint32_t i0 = perm[p0];
        for (uint32_t p = p0; p < pe; ++p) {
          const uint32_t in = p + 1 < pe ? perm[p + 1] : 0;
          x.reply((U*)out_at[frame_of(f, i0)], (uint64_t)i0 * upr + c);
          i0 = in;
        }
      }
    }
  }
}

// ---- the pooled update (psg_table_update_pooled) ------------------------------------
// base + bag_of[i] for every position i < n of the id list: the bag b with
// offsets[b] <= i < offsets[b + 1] (offsets checked: k_offsets_check).  A block
// takes kBlock bags, keeps their kBlock + 1 offsets in LDS and writes the
// stretch of positions they cover, consecutive lanes consecutive words; a lane
// finds its position's bag in 8 steps over LDS (the last offset <= i: empty bags
// share an offset with the bag behind them and own no position).  8 B read per
// bag, 4 B written per id — and a per-occurrence search of `offsets` in global
// memory is kept out of the walk's gradient chain.  base: 0, or the first
// gradient row of the list's frame in a round of several (k_row_index).
__global__ __launch_bounds__(256) void k_bag_of(const uint64_t* __restrict__ offsets, uint64_t nb, uint32_t base,
                                                uint32_t* __restrict__ bag_of) {
  __shared__ uint32_t off[kBlock + 1];
  const uint64_t ntiles = (nb + kBlock - 1) / kBlock;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t b0 = t * kBlock;
    const uint32_t nr = (uint32_t)(nb - b0 < kBlock ? nb - b0 : kBlock);
    for (uint32_t j = threadIdx.x; j <= nr; j += kBlock) off[j] = (uint32_t)offsets[b0 + j];
    __syncthreads();
    const uint32_t p1 = off[nr];
    for (uint64_t p = (uint64_t)off[0] + threadIdx.x; p < p1; p += kBlock) {  // 64 bits: p1 may be 2^32 - 2
      uint32_t lo = 0, hi = nr;  // off[lo] <= p < off[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid;
        else hi = mid;
      }
      bag_of[p] = base + (uint32_t)(b0 + lo);
    }
    __syncthreads();
  }
}

// What k_bag_of writes for a pooled frame, for a plain one (a gradient row per
// key): idx[i] = base + i for i < n.
__global__ __launch_bounds__(256) void k_row_index(uint32_t* __restrict__ idx, uint64_t n, uint32_t base) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    idx[i] = base + (uint32_t)i;
}

// Where the pooled walk finds gradient row `row`.  OneArray: in the one array of
// psg_table_update_pooled, a row per bag.  FrameArrays: in the frame that holds
// row `row` of the round's gradient arrays laid end to end
// (psg_table_update_pooled_merged): f.off[j] is the first row of frame j,
// f.vals[j] its array moved back by that many rows, so `row` indexes it as it is;
// a block keeps the addresses in LDS, as k_rows_walk_merge does.
// kPool: what an occurrence receives of its gradient row
// (psg_table_update_pooled_weighted).  WeightedArray: the row times w[p], w
// indexed as `bags` is (the walk's positions); MeanArray: the row divided by its
// bag's length, read from the checked offsets.  One f32 operation per element.
template <typename U> struct OneArray {
  static constexpr bool kFrames = false;
  static constexpr int kPool = kPoolSum;
  const U* grads;
};
struct FrameArrays {
  static constexpr bool kFrames = true;
  static constexpr int kPool = kPoolSum;
  Frames f;
};
template <typename U> struct WeightedArray {
  static constexpr bool kFrames = false;
  static constexpr int kPool = kPoolWeighted;
  const U* grads;
  const float* w;
};
template <typename U> struct MeanArray {
  static constexpr bool kFrames = false;
  static constexpr int kPool = kPoolMean;
  const U* grads;
  const uint64_t* offsets;
};

// Pass 2 of the pooled updates: k_rows_walk_merge's walk with a gradient-row
// index per occurrence.  Unique row u (slot slots[u]) for u < m; its
// occurrences are the sorted positions seg[u] .. seg[u + 1), in arrival order,
// and bags[p] is the gradient row of the occurrence at sorted position p — the
// sort carried it as its payload (k_bag_of, k_row_index), so bags IS
// bag_of[perm[.]] and the chain is bags -> gradient -> add, as the merged walk's
// is perm -> gradient -> add: the row index two ahead and the gradient unit one
// ahead are loaded before the current add.  The sum starts from +0.0f, then one
// step and one store: one writer per row, no atomics, no Pull leg.  SRC says
// where a gradient row lives: OneArray (no Frames, no frame_of, no LDS) or
// FrameArrays (frame_of over the frames' first rows: 15 compares and one 8-B
// LDS read an occurrence).  STRICT (OneArray only): the list ascends strictly,
// nothing was sorted; row u's one occurrence is position u, bags is bag_of
// itself and seg is not read.  SRC::kPool: a weighted occurrence's weight is
// loaded beside its row index, two ahead, and a mean occurrence's bag length
// beside its gradient unit, one ahead (two words of `offsets` the row's lanes
// share), so the chain stays (bags[p], w[p]) -> gradient unit -> mul -> add; the
// multiply or the division is one f32 operation and the add is the one there was.
template <typename UNIT, typename SRC, bool STRICT>
__global__ __launch_bounds__(256) void k_rows_walk_pool(typename UNIT::U* __restrict__ R, double* __restrict__ M,
                                                        const uint32_t* __restrict__ slots,
                                                        const uint32_t* __restrict__ seg,
                                                        const uint32_t* __restrict__ bags, SRC src, uint64_t m,
                                                        uint32_t upr, uint32_t rpt, typename UNIT::Params prm) {
  using U = typename UNIT::U;
  static_assert(!(STRICT && SRC::kFrames), "a round of several frames is always sorted");
  __shared__ uint64_t vals_at[kMaxFrames];  // FrameArrays only
  if constexpr (SRC::kFrames) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < kMaxFrames; ++j) vals_at[j] = (uint64_t)src.f.vals[j];
    }
    __syncthreads();
  }
  const uint64_t ntiles = (m + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t u0 = t * rpt;
    const uint32_t nr = (uint32_t)(m - u0 < rpt ? m - u0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t u = u0 + w.r;
      const uint32_t c = w.c;
      const uint32_t p0 = STRICT ? (uint32_t)u : seg[u];
      const uint32_t pe = STRICT ? (uint32_t)u + 1 : seg[u + 1];  // > p0: every unique key has an occurrence
      auto grad_at = [&](uint32_t row) {
        if constexpr (SRC::kFrames)
          return UNIT::load_grad((const U*)vals_at[frame_of(src.f, row)], (uint64_t)row * upr + c);
        else
          return UNIT::load_grad(src.grads, (uint64_t)row * upr + c);
      };
      // MeanArray: the length of gradient row `row`'s bag, as the division takes it
      [[maybe_unused]] auto len_of = [&](uint32_t row) {
        if constexpr (SRC::kPool == kPoolMean)
          return (float)(uint32_t)(src.offsets[(uint64_t)row + 1] - src.offsets[row]);
        else
          return 0.0f;
      };
      UNIT x;
      x.locate(slots[u], c, upr, prm);
      x.load_state(R, M, prm);  // issued here, used after the sum
      uint32_t b1 = p0 + 1 < pe ? bags[p0 + 1] : 0;
      [[maybe_unused]] float f = 0, f1 = 0;  // the factors of v and of the occurrence behind it
      if constexpr (SRC::kPool == kPoolWeighted) {
        f = src.w[p0];
        if (p0 + 1 < pe) f1 = src.w[p0 + 1];
      }
      const uint32_t bfirst = bags[p0];
      U v = grad_at(bfirst);
      if constexpr (SRC::kPool == kPoolMean) f = len_of(bfirst);
      U s = {};  // +0.0f
      for (uint32_t p = p0; p < pe; ++p) {
        const uint32_t b2 = p + 2 < pe ? bags[p + 2] : 0;
        [[maybe_unused]] float f2 = 0;
        if constexpr (SRC::kPool == kPoolWeighted)
          if (p + 2 < pe) f2 = src.w[p + 2];
        U vn = v;
        if (p + 1 < pe) {
          vn = grad_at(b1);
          if constexpr (SRC::kPool == kPoolMean) f1 = len_of(b1);
        }
        if constexpr (SRC::kPool == kPoolWeighted)
          s = s + f * v;
        else if constexpr (SRC::kPool == kPoolMean)
          s = s + v / f;
        else
          s = s + v;
        b1 = b2, v = vn;
        if constexpr (SRC::kPool == kPoolWeighted) f = f1, f1 = f2;
        if constexpr (SRC::kPool == kPoolMean) f = f1;
      }
      x.step(s, prm);
      x.store_state(R, M, prm);
    }
  }
}

unsigned grid_for(uint64_t blocks) {
  const uint64_t cap = (uint64_t)max_stream_blocks();
  if (blocks > cap) blocks = cap;
  return blocks ? (unsigned)blocks : 1u;
}

unsigned grid_per_lane(uint64_t n) { return grid_for((n + kBlock - 1) / kBlock); }  // one lane per element

// The geometry of every walk over rows of upr units: the rows of a tile, a block per tile.
struct Tiles {
  uint32_t rpt;
  unsigned grid;
};
Tiles tiles_for(uint64_t rows, uint32_t upr) {
  const uint32_t rpt = rows_per_tile(upr);
  return {rpt, grid_for((rows + rpt - 1) / rpt)};
}

// ---- what several calls refuse, under the call's name ----------------------------
int require_table(const char* name, const psg_table* t) {
  PSG_REQUIRE(t, PSG_ERR_INVALID, "%s: null table", name);
  return PSG_OK;
}
int require_keys(const char* name, const uint64_t* keys) {
  PSG_REQUIRE(keys, PSG_ERR_INVALID, "%s: null keys", name);
  return PSG_OK;
}
int require_count(const char* name, uint64_t n, const char* what = "keys") {
  PSG_REQUIRE(n <= kMaxRows, PSG_ERR_RANGE, "%s: more than 2^32-2 %s in one request", name, what);
  return PSG_OK;
}
// a round's keys (or gradient rows) so far and one more frame's
int require_round_count(const char* name, uint64_t N, uint64_t n, const char* what = "keys") {
  PSG_REQUIRE(n <= kMaxRows && N + n <= kMaxRows, PSG_ERR_RANGE, "%s: more than 2^32-2 %s in one round", name, what);
  return PSG_OK;
}
int require_frame_count(const char* name, int k) {
  PSG_REQUIRE(k >= 1 && k <= kMaxFrames, PSG_ERR_INVALID, "%s: %d frames outside [1, %d]", name, k, kMaxFrames);
  return PSG_OK;
}
int require_update_flags(const char* name, int flags) {
  PSG_REQUIRE(flags == PSG_PUSH || flags == (PSG_PUSH | PSG_PULL), PSG_ERR_INVALID,
              "%s: flags %d are neither PUSH nor PUSH|PULL", name, flags);
  return PSG_OK;
}
int require_iteration(const char* name, int iteration) {
  PSG_REQUIRE(iteration >= 0, PSG_ERR_INVALID, "%s: iteration %d below 0", name, iteration);
  return PSG_OK;
}
int require_f32(const char* name, const psg_table* t) {
  PSG_REQUIRE(t->dtype == PSG_F32, PSG_ERR_UNSUPPORTED, "%s: the update is built for F32 tables", name);
  return PSG_OK;
}

// ---- rows as raw bytes ------------------------------------------------------------
// f(U{}) with U the unsigned unit of unit_bytes bytes: 16, 8, 4, else 2.
template <typename F>
int for_raw_unit(uint32_t unit_bytes, F&& f) {
  switch (unit_bytes) {
    case 16: return f(u32x4{});
    case 8: return f(uint64_t{});
    case 4: return f(uint32_t{});
    default: return f(uint16_t{});
  }
}

// The table's own rows (insert, erase): 16, 4 or 2 B, whichever the row length allows; never 8.
uint32_t table_unit_bytes(const psg_table* t) {
  const uint32_t rb = t->width * (uint32_t)t->esize;
  return rb % 16 == 0 ? 16 : rb % 4 == 0 ? 4 : 2;
}

// 16-B vectors when every row, here and in the request, starts on 16 B
bool accumulate_vec(const psg_table* t, int op, const void* vals, const void* out) {
  return ((uint64_t)t->width * t->esize) % 16 == 0 && (!(op & PSG_PUSH) || aligned16(vals)) &&
         (!(op & PSG_PULL) || aligned16(out));
}

// A request's rows (assign, lookup): 16 B under accumulate_vec's condition, else the element.
uint32_t request_unit_bytes(const psg_table* t, int op, const void* vals, const void* out) {
  return accumulate_vec(t, op, vals, out) ? 16 : (uint32_t)t->esize;
}

// dst row map[j] = src row j (k_rows_move; src null: a zero row) or, take, dst
// row j = src row map[j] (k_rows_take), for j < nrows.
template <typename U>
int launch_move(bool take, const void* src, void* dst, const uint32_t* map, uint64_t nrows, uint32_t upr,
                hipStream_t st) {
  const Tiles g = tiles_for(nrows, upr);
  if (take)
    k_rows_take<U><<<g.grid, kBlock, 0, st>>>((const U*)src, (U*)dst, map, nrows, upr, g.rpt);
  else
    k_rows_move<U><<<g.grid, kBlock, 0, st>>>((const U*)src, (U*)dst, map, nrows, upr, g.rpt);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// value rows move as raw bytes (a moment row is width 16-B units: launch_move<u32x4>)
int move_rows(const psg_table* t, bool take, const void* src, void* dst, const uint32_t* map, uint64_t nrows,
              hipStream_t st) {
  const uint32_t rb = t->width * (uint32_t)t->esize;
  return for_raw_unit(table_unit_bytes(t), [&](auto u) -> int {
    using U = decltype(u);
    if constexpr (sizeof(U) == 8)
      __builtin_unreachable();  // table_unit_bytes never says 8, and no 8-B move is built
    else
      return launch_move<U>(take, src, dst, map, nrows, rb / (uint32_t)sizeof(U), st);
  });
}

inline uint64_t mom_row_bytes(const psg_table* t) { return (uint64_t)t->width * 2 * sizeof(double); }

int ensure_slots(psg_table* t, uint64_t n) {
  if (t->slots_cap >= n) return PSG_OK;
  if (t->slots) PSG_HIP(hipFree(t->slots));
  t->slots = nullptr;
  t->slots_cap = 0;
  const uint64_t cap = std::max<uint64_t>(n, 1 << 16);
  PSG_HIP(hipMalloc((void**)&t->slots, cap * sizeof(uint32_t)));
  t->slots_cap = cap;
  return PSG_OK;
}

// ---- the front half of a request ----------------------------------------------------
// Pass 1: q's slots into t->slots and its flags into `flags`.  ordered: k_rows_resolve,
// which looks at order and absence as well; else k_rows_resolve_any, for a list in any order.
int launch_resolve(psg_table* t, const uint64_t* q, uint64_t n, int* flags, bool ordered, hipStream_t st) {
  const unsigned g = grid_for((n + kRowTile - 1) / kRowTile);
  if (ordered)
    k_rows_resolve<<<g, kBlock, 0, st>>>(q, n, t->keys, t->size, t->key_begin, t->key_end, t->slots, flags);
  else
    k_rows_resolve_any<<<g, kBlock, 0, st>>>(q, n, t->keys, t->size, t->key_begin, t->key_end, t->slots, flags);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

int launch_offsets_check(const uint64_t* offsets, uint64_t n, uint64_t nb, int* flags, hipStream_t st) {
  k_offsets_check<<<grid_per_lane(nb + 1), kBlock, 0, st>>>(offsets, nb, n, flags);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// The flags on the host: t->flags_host cleared, `checks` (the pooled calls' offsets
// checks, which raise flags of their own in front of the resolve), the resolve of q where
// there are keys, one synchronisation.  Nothing is written to the table.
template <typename F>
int resolve_first(psg_table* t, const uint64_t* q, uint64_t n, bool ordered, hipStream_t st, F&& checks) {
  PSG_TRY(ensure_slots(t, n));
  memset(t->flags_host, 0, kNFlags * sizeof(int));
  PSG_TRY(checks());
  if (n) PSG_TRY(launch_resolve(t, q, n, t->flags, ordered, st));
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}
int resolve_first(psg_table* t, const uint64_t* q, uint64_t n, bool ordered, hipStream_t st) {
  return resolve_first(t, q, n, ordered, st, [] { return (int)PSG_OK; });
}

// The flags on the device (the lookups): t->gate (kNFlags ints, on first use) cleared on
// the stream; the caller's checks, resolve and walk raise and read it with no host in
// between; gate_end copies it to t->flags_host and is the call's one synchronisation.
int gate_begin(psg_table* t, uint64_t n, hipStream_t st) {
  PSG_TRY(ensure_slots(t, n));
  if (!t->gate) PSG_HIP(hipMalloc((void**)&t->gate, kNFlags * sizeof(int)));
  PSG_HIP(hipMemsetAsync(t->gate, 0, kNFlags * sizeof(int), st));
  return PSG_OK;
}
int gate_end(psg_table* t, hipStream_t st) {
  PSG_HIP(hipMemcpyAsync(t->flags_host, t->gate, kNFlags * sizeof(int), hipMemcpyDeviceToHost, st));
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

int require_ascending(const psg_table* t) {
  PSG_REQUIRE(!t->flags_host[R_UNSORTED], PSG_ERR_INVALID,
              "request keys are not strictly ascending (KVPairs contract, KVApp.h:23)");
  return PSG_OK;
}

int require_in_range(const psg_table* t) {
  PSG_REQUIRE(!t->flags_host[R_RANGE], PSG_ERR_RANGE, "request key outside the table range [%llu, %llu)",
              (unsigned long long)t->key_begin, (unsigned long long)t->key_end);
  return PSG_OK;
}

int require_offsets(const psg_table* t, const char* name, uint64_t n) {
  PSG_REQUIRE(!t->flags_host[R_OFFSETS], PSG_ERR_INVALID,
              "%s: offsets do not start at 0, ascend and end at n = %llu", name, (unsigned long long)n);
  return PSG_OK;
}

struct DevBuf {  // a device scratch array freed on every return path
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// New arrays of `size` rows in `cap` take the table's place (insert, erase);
// the old ones are left in K2 / R2 / M2 and freed with them.
void publish_arrays(psg_table* t, DevBuf& K2, DevBuf& R2, DevBuf& M2, uint64_t size, uint64_t cap) {
  void* old_keys = t->keys;
  t->keys = (uint64_t*)K2.p;
  K2.p = old_keys;
  std::swap(R2.p, t->rows);
  if (t->adam) {
    void* old_mom = t->mom;
    t->mom = (double*)M2.p;
    M2.p = old_mom;
  }
  t->size = size;
  t->capacity = cap;
}

// ---- the initial rows: what the host passes ----------------------------------------
inline bool has_init(const psg_table* t) { return t->init_kind == PSG_INIT_UNIFORM; }
inline InitSpec init_spec(uint64_t seed, float lo, float hi) {
  return {(uint32_t)seed, (uint32_t)(seed >> 32), lo, hi - lo};
}
inline InitSpec init_spec(const psg_table* t) { return init_spec(t->init_seed, t->init_lo, t->init_hi); }
// what psg_table_set_init and psg_init_rows refuse of a uniform range, in the header's order
int require_uniform(const char* name, float lo, float hi) {
  PSG_REQUIRE(std::isfinite(lo) && std::isfinite(hi), PSG_ERR_INVALID, "%s: lo %g or hi %g is not finite", name, lo, hi);
  PSG_REQUIRE(lo <= hi, PSG_ERR_INVALID, "%s: lo %g above hi %g", name, lo, hi);
  const volatile float span = hi - lo;
  PSG_REQUIRE(std::isfinite(span), PSG_ERR_INVALID, "%s: hi - lo is not finite in f32", name);
  return PSG_OK;
}
// The initial rows of keys[0 .. nrows) into dst: row to[j], or row j where `to`
// is null.  vec: rows of a multiple of 16 B that start on 16 B.
int launch_init(int dtype, uint32_t width, void* dst, const uint64_t* keys, const uint32_t* to, uint64_t nrows,
                bool vec, const InitSpec& spec, hipStream_t st);

// Insert the keys of q that t->slots marks absent, each with a zero row or,
// where the table has an initializer, its initial row.
int insert_missing(psg_table* t, const uint64_t* q, uint64_t n, hipStream_t st) {
  const uint64_t ntiles = compact_tiles(n);
  const SlotIs absent = {t->slots, kAbsent};
  DevBuf counts, miss, old_to, new_to;
  PSG_HIP(hipMalloc(&counts.p, (ntiles + 1) * sizeof(uint32_t)));
  compact_count(n, (uint32_t*)counts.p, absent, st);
  PSG_HIP(hipGetLastError());
  uint64_t m = 0;
  PSG_TRY(read_count((const uint32_t*)counts.p + ntiles, &m, st));
  const uint64_t S = t->size;
  if (m == 0) return PSG_OK;
  uint64_t cap = t->capacity;
  if (S + m > cap) cap = std::max<uint64_t>(std::max<uint64_t>(S + m, cap * 2), 1024);
  if (cap > kMaxRows) cap = kMaxRows;
  PSG_REQUIRE(S + m <= kMaxRows, PSG_ERR_RANGE, "psg_table: more than 2^32-2 rows");
  const uint64_t row_bytes = (uint64_t)t->width * t->esize;
  PSG_HIP(hipMalloc(&miss.p, m * sizeof(uint64_t)));
  PSG_HIP(hipMalloc(&old_to.p, std::max<uint64_t>(S, 1) * sizeof(uint32_t)));
  PSG_HIP(hipMalloc(&new_to.p, m * sizeof(uint32_t)));
  compact_emit(n, (const uint32_t*)counts.p, absent, EmitKey{q, (uint64_t*)miss.p}, st);
  PSG_HIP(hipGetLastError());
  DevBuf K2, R2, M2;
  PSG_HIP(hipMalloc(&K2.p, cap * sizeof(uint64_t)));
  PSG_HIP(hipMalloc(&R2.p, cap * row_bytes));
  if (t->adam) PSG_HIP(hipMalloc(&M2.p, cap * mom_row_bytes(t)));
  k_rows_merge_keys<<<grid_per_lane(S + m), kBlock, 0, st>>>(t->keys, S, (const uint64_t*)miss.p, m, (uint64_t*)K2.p,
                                                            (uint32_t*)old_to.p, (uint32_t*)new_to.p);
  PSG_HIP(hipGetLastError());
  if (S) PSG_TRY(move_rows(t, false, t->rows, R2.p, (const uint32_t*)old_to.p, S, st));
  if (has_init(t))
    PSG_TRY(launch_init(t->dtype, t->width, R2.p, (const uint64_t*)miss.p, (const uint32_t*)new_to.p, m,
                        row_bytes % 16 == 0, init_spec(t), st));
  else
    PSG_TRY(move_rows(t, false, nullptr, R2.p, (const uint32_t*)new_to.p, m, st));
  if (t->adam) {  // the moment rows go where their value rows went: 2 * width doubles = width 16-B units
    if (S) PSG_TRY(launch_move<u32x4>(false, t->mom, M2.p, (const uint32_t*)old_to.p, S, t->width, st));
    PSG_TRY(launch_move<u32x4>(false, nullptr, M2.p, (const uint32_t*)new_to.p, m, t->width, st));
  }
  PSG_HIP(hipStreamSynchronize(st));
  publish_arrays(t, K2, R2, M2, S + m, cap);
  return PSG_OK;
}

// Behind resolve_first's flags of a strictly ascending list in range: insert its
// absent keys and resolve again.
int resolve_finish(psg_table* t, const uint64_t* keys, uint64_t n, hipStream_t st) {
  if (t->flags_host[R_MISSING]) {
    PSG_TRY(insert_missing(t, keys, n, st));
    PSG_TRY(resolve_first(t, keys, n, true, st));
    PSG_REQUIRE(!t->flags_host[R_MISSING], PSG_ERR_HIP, "psg_table: a key is absent after its insert");
  }
  return PSG_OK;
}

// The whole front half as a strict call does it: a bad list is rejected before
// anything is written.  plan_any resolves its unique list this way.
int resolve_request(psg_table* t, const uint64_t* keys, uint64_t n, hipStream_t st) {
  PSG_TRY(resolve_first(t, keys, n, true, st));
  PSG_TRY(require_ascending(t));
  PSG_TRY(require_in_range(t));
  return resolve_finish(t, keys, n, st);
}

// ---- the order-preserving request ---------------------------------------------
struct AnyScratch {
  uint64_t *k0, *k1;       // the sort's key buffers; afterwards the sorted keys and U
  uint32_t *p0, *p1;       // the sort's position buffers; afterwards perm
  uint32_t *seg, *counts;  // seg[n + 1]; radix counts, then the head counts per tile
};

int any_scratch(psg_table* t, uint64_t n, AnyScratch* a) {
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  const uint64_t ntiles = compact_tiles(n);
  const uint64_t u64n = al(n * 8), u32n = al(n * 4), segb = al((n + 1) * 4);
  const uint64_t cnt = al(std::max<uint64_t>(radix_counts_elems(n), ntiles + 1) * 4);
  const uint64_t bytes = 2 * u64n + 2 * u32n + segb + cnt;
  if (t->any_bytes < bytes) {
    if (t->any_buf) PSG_HIP(hipFree(t->any_buf));
    t->any_buf = nullptr;
    t->any_bytes = 0;
    const uint64_t cap = std::max<uint64_t>(bytes + bytes / 2, 1 << 20);
    PSG_HIP(hipMalloc(&t->any_buf, cap));
    t->any_bytes = cap;
  }
  char* p = (char*)t->any_buf;
  a->k0 = (uint64_t*)p, p += u64n;
  a->k1 = (uint64_t*)p, p += u64n;
  a->p0 = (uint32_t*)p, p += u32n;
  a->p1 = (uint32_t*)p, p += u32n;
  a->seg = (uint32_t*)p, p += segb;
  a->counts = (uint32_t*)p;
  return PSG_OK;
}

// A key list into the sort's key buffer, `first` keys in (a round lays its frames' lists
// end to end).  The sort permutes the buffer: a copy, the caller's keys are never written.
int copy_keys(const AnyScratch& a, uint64_t first, const uint64_t* keys, uint64_t n, hipStream_t st) {
  if (n) PSG_HIP(hipMemcpyAsync(a.k0 + first, keys, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  return PSG_OK;
}

// A round's frame table before its k frames are filled in: from k on, offsets no position reaches.
Frames round_frames(int k) {
  Frames f = {};
  f.k = k;
  for (int j = k; j <= kMaxFrames; ++j) f.off[j] = 0xffffffffu;
  return f;
}

// A frame's array of F32 rows moved back by the frame's first row in the round,
// so that a row of the frames laid end to end indexes it as it is.
template <typename T>
T* moved_back(const psg_table* t, T* rows, uint32_t first) {
  return (T*)((uintptr_t)rows - first * ((uint64_t)t->width * sizeof(float)));
}

int bit_width(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; }

struct AnyPlan {  // the request as unique rows: slots in t->slots[m]
  uint64_t m;
  const uint32_t *seg, *perm;
};

// The n keys in a.k0, all in range: sort (key, position) stably, cut the runs
// of equal keys, resolve the unique list as a strict request.  payload: the
// sort carries the n words the caller left in a.p0 instead of the positions,
// and plan->perm holds them in sorted order (the pooled update's bags).
int plan_scratch(psg_table* t, const AnyScratch& a, uint64_t n, AnyPlan* plan, hipStream_t st, bool payload = false) {
  int res = 0;
  const int bits = std::max(1, bit_width(t->key_end - 1));  // every key is below key_end
  PSG_TRY(radix_sort_u64(a.k0, a.p0, n, bits, !payload, a.k1, a.p1, a.counts, st, &res));
  const uint64_t* sorted = res ? a.k1 : a.k0;
  uint64_t* U = res ? a.k0 : a.k1;
  compact_count(n, a.counts, RunHead{sorted}, st);
  compact_emit(n, a.counts, RunHead{sorted}, EmitHead{sorted, n, U, a.seg}, st);
  PSG_HIP(hipGetLastError());
  uint64_t m = 0;
  PSG_TRY(read_count(a.counts + compact_tiles(n), &m, st));
  PSG_REQUIRE(m >= 1 && m <= n, PSG_ERR_HIP, "psg_table: %u unique keys in a list of %llu", (uint32_t)m,
              (unsigned long long)n);
  PSG_TRY(resolve_request(t, U, m, st));
  plan->m = m;
  plan->seg = a.seg;
  plan->perm = res ? a.p1 : a.p0;
  return PSG_OK;
}

// A list in range that is not strictly ascending.
int plan_any(psg_table* t, const uint64_t* keys, uint64_t n, AnyPlan* plan, hipStream_t st) {
  AnyScratch a;
  PSG_TRY(any_scratch(t, n, &a));
  PSG_TRY(copy_keys(a, 0, keys, n, st));
  return plan_scratch(t, a, n, plan, st);
}

// ---- pass 2: the dispatch -----------------------------------------------------------
// Either walk for one unit type and op: the strict one over the request's n
// rows (plan null), or the segment walk over the plan's unique rows.
template <typename UNIT, int OP>
int launch_walk(psg_table* t, const AnyPlan* p, const void* vals, void* out, uint64_t n, uint32_t upr,
                const typename UNIT::Params& prm, hipStream_t st) {
  using U = typename UNIT::U;
  const Tiles g = tiles_for(p ? p->m : n, upr);
  if (p)
    k_rows_walk_seg<UNIT, OP><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, p->seg, p->perm,
                                                          (const U*)vals, (U*)out, p->m, upr, g.rpt, prm);
  else
    k_rows_walk<UNIT, OP><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, (const U*)vals, (U*)out, n, upr,
                                                      g.rpt, prm);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

template <typename UNIT>
int launch_op(psg_table* t, int op, const AnyPlan* p, const void* vals, void* out, uint64_t n, uint32_t upr,
              const typename UNIT::Params& prm, hipStream_t st) {
  if (op == PSG_PUSH) return launch_walk<UNIT, PSG_PUSH>(t, p, vals, out, n, upr, prm, st);
  if constexpr (UNIT::kPullAlone)
    if (op == PSG_PULL) return launch_walk<UNIT, PSG_PULL>(t, p, vals, out, n, upr, prm, st);
  return launch_walk<UNIT, PSG_PUSH | PSG_PULL>(t, p, vals, out, n, upr, prm, st);
}

// f(dt) with decltype(dt)::value the table's dtype
template <typename F>
int with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case PSG_F32: return f(std::integral_constant<int, PSG_F32>{});
    case PSG_F64: return f(std::integral_constant<int, PSG_F64>{});
    case PSG_F16: return f(std::integral_constant<int, PSG_F16>{});
    default: return f(std::integral_constant<int, PSG_BF16>{});
  }
}

int launch_init(int dtype, uint32_t width, void* dst, const uint64_t* keys, const uint32_t* to, uint64_t nrows,
                bool vec, const InitSpec& spec, hipStream_t st) {
  return with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const uint32_t upr = vec ? width / Elem<DT>::kVec : (width + 3) / 4;  // 16-B units, or blocks of four elements
    const Tiles g = tiles_for(nrows, upr);
    if (vec)
      k_rows_init<DT, true><<<g.grid, kBlock, 0, st>>>((typename InitUnit<DT, true>::U*)dst, keys, to, nrows, width, upr,
                                                       g.rpt, spec);
    else
      k_rows_init<DT, false><<<g.grid, kBlock, 0, st>>>((typename InitUnit<DT, false>::U*)dst, keys, to, nrows, width,
                                                        upr, g.rpt, spec);
    PSG_HIP(hipGetLastError());
    return (int)PSG_OK;
  });
}

int accumulate(psg_table* t, int op, const AnyPlan* p, const void* vals, void* out, uint64_t n, hipStream_t st) {
  const bool vec = accumulate_vec(t, op, vals, out);
  return with_dtype(t->dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (vec) return launch_op<AccUnit<DT, true>>(t, op, p, vals, out, n, t->width / Elem<DT>::kVec, {}, st);
    return launch_op<AccUnit<DT, false>>(t, op, p, vals, out, n, t->width, {}, st);
  });
}

// 16-B units of an update: four columns, every gradient and reply array on 16 B
bool optimize_vec(const psg_table* t, int op, const float* grads, const float* out) {
  return t->width % 4 == 0 && aligned16(grads) && (!(op & PSG_PULL) || aligned16(out));
}

// The two bias corrections of Adam.h:31-32, once for the request, with the host
// libm pow the reference calls (as psg_lr.hip).  Zeros for an SGD table.
AdamArgs adam_args(const psg_table* t, int iteration) {
  if (!t->adam) return {};
  return {t->alr,  t->beta1, t->beta2, t->eps, 1 - std::pow(t->beta1, iteration + 1),
          1 - std::pow(t->beta2, iteration + 1)};
}

// f(unit, upr, prm) for the table's optimizer unit: unit is a UnitTag of
// OptUnit<ADAM, VEC> (ADAM: the table has Adam state; VEC: the caller's vec),
// upr its units per row and prm its Params, built once for the request.
template <typename UNIT> struct UnitTag {
  using type = UNIT;
};
template <typename F>
int with_opt_unit(const psg_table* t, bool vec, float lr, int iteration, F&& f) {
  const AdamArgs a = adam_args(t, iteration);
  auto with = [&](auto unit) {
    using UNIT = typename decltype(unit)::type;
    return f(unit, vec ? t->width / 4 : t->width, typename UNIT::Params{t->width, lr, a});
  };
  if (t->adam) return vec ? with(UnitTag<OptUnit<true, true>>{}) : with(UnitTag<OptUnit<true, false>>{});
  return vec ? with(UnitTag<OptUnit<false, true>>{}) : with(UnitTag<OptUnit<false, false>>{});
}

// The body of the four request calls; `name` is the call's, for its messages.
// opt: psg_table_update* (vals are gradients) instead of psg_table_handle*;
// any: a list that is not strictly ascending is planned instead of rejected.
int serve(const char* name, bool opt, bool any, psg_table* t, int flags, const uint64_t* keys, const void* vals,
          void* out, uint64_t n, float lr, int iteration, psg_stream stream) {
  PSG_TRY(require_table(name, t));
  if (opt) {
    PSG_TRY(require_update_flags(name, flags));
    PSG_TRY(require_iteration(name, iteration));
    PSG_TRY(require_f32(name, t));
  } else {
    PSG_REQUIRE(flags >= 1 && flags <= 3, PSG_ERR_INVALID, "%s: bad flags %d", name, flags);
  }
  if (n == 0) return PSG_OK;
  PSG_TRY(require_keys(name, keys));
  if (opt)
    PSG_REQUIRE(vals, PSG_ERR_INVALID, "%s: null grads", name);
  else
    PSG_REQUIRE(!(flags & PSG_PUSH) || vals, PSG_ERR_INVALID, "push without vals");
  PSG_REQUIRE(!(flags & PSG_PULL) || out, PSG_ERR_INVALID, "pull without out buffer");
  PSG_TRY(require_count(name, n));
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(resolve_first(t, keys, n, true, st));
  // a strict call rejects a list out of order before it looks at the range
  if (!any) PSG_TRY(require_ascending(t));
  PSG_TRY(require_in_range(t));
  AnyPlan plan;
  const AnyPlan* p = nullptr;
  if (t->flags_host[R_UNSORTED]) {
    PSG_TRY(plan_any(t, keys, n, &plan, st));
    p = &plan;
  } else {
    PSG_TRY(resolve_finish(t, keys, n, st));
  }
  if (opt) {
    const bool vec = optimize_vec(t, flags, (const float*)vals, (const float*)out);
    PSG_TRY(with_opt_unit(t, vec, lr, iteration, [&](auto unit, uint32_t upr, const auto& prm) {
      return launch_op<typename decltype(unit)::type>(t, flags, p, vals, out, n, upr, prm, st);
    }));
  } else {
    PSG_TRY(accumulate(t, flags, p, vals, out, n, st));
  }
  // complete on return: keys and vals no longer read, a Pull's reply in memory
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

// ---- assign and export -----------------------------------------------------------
// The moments of n request rows (slots: t->slots, or null for the table's rows
// first .. first + n) between the table and the plain arrays m, v.
template <bool TO_TABLE>
int move_moments(psg_table* t, const uint32_t* slots, uint64_t first, const double* m, const double* v, uint64_t n,
                 hipStream_t st) {
  const bool pair = t->width % 4 == 0 && aligned16(m) && aligned16(v);
  const Tiles g = tiles_for(n, pair ? t->width : 2 * t->width);
  double* mp = const_cast<double*>(m);
  double* vp = const_cast<double*>(v);
  if (pair)
    k_mom_move<f64x2, TO_TABLE><<<g.grid, kBlock, 0, st>>>(t->mom, slots, first, mp, vp, n, t->width, g.rpt);
  else
    k_mom_move<double, TO_TABLE><<<g.grid, kBlock, 0, st>>>(t->mom, slots, first, mp, vp, n, t->width, g.rpt);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

template <typename U>
int launch_set(psg_table* t, const void* rows, uint64_t n, uint32_t upr, hipStream_t st) {
  const Tiles g = tiles_for(n, upr);
  k_rows_walk<SetUnit<U>, PSG_PUSH><<<g.grid, kBlock, 0, st>>>((U*)t->rows, nullptr, t->slots, (const U*)rows, nullptr,
                                                               n, upr, g.rpt, typename SetUnit<U>::Params{});
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// ---- lookup and erase: the calls that never insert ---------------------------------
// out null: presence alone, one lane per row
template <typename U>
int launch_read(psg_table* t, void* out, uint8_t* found, uint64_t n, uint32_t upr, hipStream_t st) {
  const Tiles g = tiles_for(n, upr);
  k_rows_read<U><<<out ? g.grid : grid_per_lane(n), kBlock, 0, st>>>((const U*)t->rows, t->slots, (U*)out, found, n, upr,
                                                                    g.rpt, t->gate);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// the lookup of a table with an initializer: absent ids answer with their initial rows
template <int DT, bool VEC>
int launch_read_init(psg_table* t, const uint64_t* keys, void* out, uint8_t* found, uint64_t n, uint32_t upr,
                     hipStream_t st) {
  using U = typename InitUnit<DT, VEC>::U;
  const Tiles g = tiles_for(n, upr);
  k_rows_read_init<DT, VEC><<<g.grid, kBlock, 0, st>>>((const U*)t->rows, t->slots, keys, (U*)out, found, n, upr, g.rpt,
                                                       t->gate, init_spec(t));
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// ---- the merged update: dispatch --------------------------------------------------
// The same-list walk over the n rows of list 0 (plan null), or the merge walk
// over the plan's unique rows.
template <typename UNIT, int OP>
int launch_merged(psg_table* t, const AnyPlan* p, const Frames& f, uint64_t n, uint32_t upr,
                  const typename UNIT::Params& prm, hipStream_t st) {
  using U = typename UNIT::U;
  const Tiles g = tiles_for(p ? p->m : n, upr);
  if (p)
    k_rows_walk_merge<UNIT, OP><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, p->seg, p->perm, f, p->m, upr,
                                                            g.rpt, prm);
  else
    k_rows_walk_same<UNIT, OP><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, f, n, upr, g.rpt, prm);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// Are the further key lists, over their first n keys, element for element list
// 0 (and, with `order`, does list 0 ascend strictly there)?  The answer is
// t->flags_host[R_DIFFER], which the caller or the resolve before has cleared.
int keys_differ(psg_table* t, int k, const uint64_t* const* keys, uint64_t n, bool order, hipStream_t st) {
  KeyFrames kf = {};
  kf.k = k;
  bool any = order;
  for (int j = 0; j < k; ++j) {
    kf.p[j] = keys[j];
    any = any || keys[j] != keys[0];
  }
  if (!any) return PSG_OK;
  k_keys_differ<<<grid_per_lane(n), kBlock, 0, st>>>(kf, n, order ? 1 : 0, t->flags);
  PSG_HIP(hipGetLastError());
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

// ---- the pooled calls: dispatch and bodies -------------------------------------------
// What both refuse before any device call, in the header's order; `rows` is the
// forward's out or the backward's grads.
int pooled_args(const char* name, const psg_table* t, const uint64_t* keys, const uint64_t* offsets, const void* rows,
                const char* rows_name, uint64_t n, uint64_t nb) {
  PSG_TRY(require_table(name, t));
  PSG_REQUIRE(keys || n == 0, PSG_ERR_INVALID, "%s: null keys", name);
  PSG_REQUIRE(offsets || nb == 0, PSG_ERR_INVALID, "%s: null offsets", name);
  PSG_REQUIRE(rows || nb == 0, PSG_ERR_INVALID, "%s: null %s", name, rows_name);
  PSG_REQUIRE(nb > 0 || n == 0, PSG_ERR_INVALID, "%s: %llu keys and no bag to hold them", name,
              (unsigned long long)n);
  return PSG_OK;
}

// What the weighted calls refuse behind pooled_args; the unweighted calls come
// through with no weights and PSG_POOL_SUM.
int pool_mode_args(const char* name, const float* weights, int mode) {
  PSG_REQUIRE(mode == PSG_POOL_SUM || mode == PSG_POOL_MEAN, PSG_ERR_INVALID, "%s: mode %d is no pooling mode", name,
              mode);
  PSG_REQUIRE(mode != PSG_POOL_MEAN || !weights, PSG_ERR_INVALID, "%s: weights with PSG_POOL_MEAN", name);
  PSG_REQUIRE((reinterpret_cast<uintptr_t>(weights) & 3u) == 0, PSG_ERR_INVALID, "%s: weights not on a 4-B boundary",
              name);
  return PSG_OK;
}

// pool: kPoolSum is the unweighted call's kernel, launched as it was
template <int DT, bool VEC>
int launch_pool(psg_table* t, const uint64_t* offsets, const float* weights, int pool, void* out, uint64_t nb,
                uint32_t upr, hipStream_t st) {
  using ACC = PoolAcc<DT, VEC>;
  using U = typename ACC::U;
  const Tiles g = tiles_for(nb, upr);
  if (pool == kPoolWeighted)
    k_rows_pool<U, ACC, kPoolWeighted><<<g.grid, kBlock, 0, st>>>((const U*)t->rows, t->slots, offsets, (U*)out, nb, upr,
                                                                  g.rpt, t->gate, weights);
  else if (pool == kPoolMean)
    k_rows_pool<U, ACC, kPoolMean><<<g.grid, kBlock, 0, st>>>((const U*)t->rows, t->slots, offsets, (U*)out, nb, upr,
                                                              g.rpt, t->gate);
  else
    k_rows_pool<U, ACC><<<g.grid, kBlock, 0, st>>>((const U*)t->rows, t->slots, offsets, (U*)out, nb, upr, g.rpt,
                                                   t->gate);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// launch_pool for a table with an initializer
template <int DT, bool VEC>
int launch_pool_init(psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* weights, int pool,
                     void* out, uint64_t nb, uint32_t upr, hipStream_t st) {
  using U = typename PoolAcc<DT, VEC>::U;
  const Tiles g = tiles_for(nb, upr);
  const InitSpec spec = init_spec(t);
  auto launch = [&](auto mode) {
    k_rows_pool_init<DT, VEC, decltype(mode)::value><<<g.grid, kBlock, 0, st>>>(
        (const U*)t->rows, t->slots, keys, offsets, (U*)out, nb, upr, g.rpt, t->gate, weights, spec);
  };
  if (pool == kPoolWeighted)
    launch(std::integral_constant<int, kPoolWeighted>{});
  else if (pool == kPoolMean)
    launch(std::integral_constant<int, kPoolMean>{});
  else
    launch(std::integral_constant<int, kPoolSum>{});
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

int lookup_pooled(const char* name, psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* weights,
                  int mode, void* out, uint64_t n, uint64_t nb, psg_stream stream) {
  PSG_TRY(pooled_args(name, t, keys, offsets, out, "out", n, nb));
  PSG_TRY(pool_mode_args(name, weights, mode));
  PSG_TRY(require_count(name, n));
  PSG_TRY(require_count(name, nb, "bags"));
  if (nb == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(gate_begin(t, n, st));
  PSG_TRY(launch_offsets_check(offsets, n, nb, t->gate, st));
  if (n) PSG_TRY(launch_resolve(t, keys, n, t->gate, false, st));
  const int pool = mode == PSG_POOL_MEAN ? kPoolMean : weights ? kPoolWeighted : kPoolSum;
  // 16-B units under accumulate_vec's condition for a Pull (the weights are read as words either way)
  const bool vec = accumulate_vec(t, PSG_PULL, nullptr, out);
  PSG_TRY(with_dtype(t->dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (has_init(t)) {
      if (vec) return launch_pool_init<DT, true>(t, keys, offsets, weights, pool, out, nb, t->width / Elem<DT>::kVec, st);
      return launch_pool_init<DT, false>(t, keys, offsets, weights, pool, out, nb, t->width, st);
    }
    if (vec) return launch_pool<DT, true>(t, offsets, weights, pool, out, nb, t->width / Elem<DT>::kVec, st);
    return launch_pool<DT, false>(t, offsets, weights, pool, out, nb, t->width, st);
  }));
  // the one synchronisation: keys, offsets and weights no longer read, the reply in memory, the flags on the host
  PSG_TRY(gate_end(t, st));
  PSG_TRY(require_offsets(t, name, n));
  return require_in_range(t);
}

// The pooled walk for one unit type and one source of gradient rows (src:
// OneArray, WeightedArray, MeanArray or, always with a plan, FrameArrays): over
// the plan's unique rows with bags[p] the gradient row of sorted position p, or
// without a plan the strict walk over the list's n rows with bags = bag_of.
template <typename UNIT, typename SRC>
int launch_walk_src(psg_table* t, const AnyPlan* p, const uint32_t* bags, const SRC& src, uint64_t n, uint32_t upr,
                    const typename UNIT::Params& prm, hipStream_t st) {
  using U = typename UNIT::U;
  if constexpr (SRC::kFrames) PSG_REQUIRE(p, PSG_ERR_INVALID, "psg_table: a round of frames without a plan");
  const Tiles g = tiles_for(p ? p->m : n, upr);
  if (p) {
    k_rows_walk_pool<UNIT, SRC, false><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, p->seg, bags, src, p->m,
                                                                  upr, g.rpt, prm);
  } else if constexpr (!SRC::kFrames) {
    k_rows_walk_pool<UNIT, SRC, true><<<g.grid, kBlock, 0, st>>>((U*)t->rows, t->mom, t->slots, nullptr, bags, src, n, upr,
                                                                 g.rpt, prm);
  }
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// What the pooled update's occurrences receive of their gradient rows: the row
// (no weights, no offsets), the row times weights[.] at the walk's positions, or
// the row over its bag's length.
struct PoolScale {
  const float* weights;
  const uint64_t* offsets;
};

// The gradient rows in the round's frames (f not null: always a plan, no scale) or in the
// one array `grads`; bags: the walk's row indices where the sort did not carry them (p->perm).
template <typename UNIT>
int launch_walk_pool(psg_table* t, const AnyPlan* p, const uint32_t* bags, const float* grads, const Frames* f,
                     const PoolScale& sc, uint64_t n, uint32_t upr, const typename UNIT::Params& prm, hipStream_t st) {
  using U = typename UNIT::U;
  if (f) return launch_walk_src<UNIT>(t, p, p->perm, FrameArrays{*f}, n, upr, prm, st);
  if (sc.weights) return launch_walk_src<UNIT>(t, p, bags, WeightedArray<U>{(const U*)grads, sc.weights}, n, upr, prm, st);
  if (p) bags = p->perm;
  if (sc.offsets) return launch_walk_src<UNIT>(t, p, bags, MeanArray<U>{(const U*)grads, sc.offsets}, n, upr, prm, st);
  return launch_walk_src<UNIT>(t, p, bags, OneArray<U>{(const U*)grads}, n, upr, prm, st);
}

// vec: 16-B units (optimize_vec's condition for a Push, on every gradient array)
int pooled_step(psg_table* t, bool vec, const AnyPlan* p, const uint32_t* bags, const float* grads, const Frames* f,
                const PoolScale& sc, uint64_t n, float lr, int iteration, hipStream_t st) {
  return with_opt_unit(t, vec, lr, iteration, [&](auto unit, uint32_t upr, const auto& prm) {
    return launch_walk_pool<typename decltype(unit)::type>(t, p, bags, grads, f, sc, n, upr, prm, st);
  });
}

// bags[p] = bag_of[perm[p]] and w[p] = weights[perm[p]] for p < n: the weighted
// update's two per-occurrence words in sorted order, gathered once behind the
// sort so that the walk reads both at its own position, as it reads the sort's
// payload, and not through perm (one more dependent load an occurrence).
// 4 B read in order and 8 B gathered per id, 8 B written in order.
__global__ __launch_bounds__(256) void k_pool_gather(const uint32_t* __restrict__ perm,
                                                     const uint32_t* __restrict__ bag_of,
                                                     const float* __restrict__ weights, uint32_t* __restrict__ bags,
                                                     float* __restrict__ w, uint64_t n) {
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = perm[p];  // a position of the list: the sort permutes 0 .. n - 1
    bags[p] = bag_of[i];
    w[p] = weights[i];
  }
}

// path (may be null): how the list was served, as psg_table_update_merged reports it.
// weights, mode: psg_table_update_pooled_weighted's; the unweighted callers pass
// none and PSG_POOL_SUM.
int update_pooled(const char* name, psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* weights,
                  int mode, const float* grads, uint64_t n, uint64_t nb, float lr, int iteration, psg_stream stream,
                  int* path) {
  PSG_TRY(pooled_args(name, t, keys, offsets, grads, "grads", n, nb));
  PSG_TRY(pool_mode_args(name, weights, mode));
  PSG_TRY(require_iteration(name, iteration));
  PSG_TRY(require_count(name, n));
  PSG_TRY(require_count(name, nb, "bags"));
  PSG_TRY(require_f32(name, t));
  if (nb == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  // the offsets check in front of the resolve: both raise their flags in
  // t->flags_host, read after one synchronisation; nothing is written yet
  PSG_TRY(resolve_first(t, keys, n, true, st, [&] { return launch_offsets_check(offsets, n, nb, t->flags, st); }));
  PSG_TRY(require_offsets(t, name, n));
  PSG_TRY(require_in_range(t));
  if (n == 0) return PSG_OK;  // every bag is empty: no gradient row is read
  // bag_of goes where the sort keeps its positions (a.p0): the sorted path sorts
  // (key, bag) pairs, the strict one reads it as it is
  const bool strict = !t->flags_host[R_UNSORTED];  // as PSG_MERGED_SAME_LIST is decided for k = 1
  AnyScratch a;
  PSG_TRY(any_scratch(t, n, &a));
  // a weighted list out of order: the sort carries positions, and bag_of is
  // written behind it, where the sort's other position buffer is free
  const bool by_position = weights && !strict;
  const uint32_t* bags = a.p0;  // what the walk reads at its positions (sorted path, unweighted: plan.perm)
  PoolScale sc = {weights, mode == PSG_POOL_MEAN ? offsets : nullptr};
  if (!by_position) {
    k_bag_of<<<grid_per_lane(nb), kBlock, 0, st>>>(offsets, nb, 0, a.p0);
    PSG_HIP(hipGetLastError());
  }
  AnyPlan plan;
  const AnyPlan* p = nullptr;
  if (strict) {
    PSG_TRY(resolve_finish(t, keys, n, st));
  } else {
    PSG_TRY(copy_keys(a, 0, keys, n, st));
    PSG_TRY(plan_scratch(t, a, n, &plan, st, !by_position));
    p = &plan;
  }
  if (by_position) {
    // behind plan_scratch on the stream both key buffers are spent (the sorted
    // keys are cut into runs, the unique list is resolved): a.k0's 8 n bytes
    // take the two gathered arrays, n words each
    uint32_t* bag_of = plan.perm == a.p0 ? a.p1 : a.p0;
    uint32_t* sorted_bags = (uint32_t*)a.k0;
    float* sorted_w = (float*)(sorted_bags + n);
    k_bag_of<<<grid_per_lane(nb), kBlock, 0, st>>>(offsets, nb, 0, bag_of);
    PSG_HIP(hipGetLastError());
    k_pool_gather<<<grid_per_lane(n), kBlock, 0, st>>>(plan.perm, bag_of, weights, sorted_bags, sorted_w, n);
    PSG_HIP(hipGetLastError());
    bags = sorted_bags;
    sc.weights = sorted_w;
  }
  const bool vec = optimize_vec(t, PSG_PUSH, grads, nullptr);
  PSG_TRY(pooled_step(t, vec, p, bags, grads, nullptr, sc, n, lr, iteration, st));
  // complete on return: keys, offsets, weights and grads no longer read
  PSG_HIP(hipStreamSynchronize(st));
  if (path) *path = strict ? PSG_MERGED_SAME_LIST : PSG_MERGED_SORTED;
  return PSG_OK;
}

}  // namespace
}  // namespace psg

using namespace psg;

extern "C" {

int psg_table_create(int dtype, uint32_t width, uint64_t key_begin, uint64_t key_end, uint64_t capacity,
                     psg_table** out) {
  PSG_REQUIRE(out, PSG_ERR_INVALID, "psg_table_create: null out");
  *out = nullptr;
  const int es = dtype_size(dtype);
  PSG_REQUIRE(es > 0, PSG_ERR_INVALID, "psg_table_create: bad dtype %d", dtype);
  PSG_REQUIRE(width >= 1 && width <= 4096, PSG_ERR_INVALID, "psg_table_create: width %u outside [1, 4096]", width);
  PSG_REQUIRE(key_begin < key_end, PSG_ERR_INVALID, "psg_table_create: empty key range");
  PSG_REQUIRE(capacity <= kMaxRows, PSG_ERR_RANGE, "psg_table_create: capacity above 2^32-2 rows");
  psg_table* t = new psg_table();  // value-initialised: every field zero
  t->dtype = dtype;
  t->esize = es;
  t->width = width;
  t->key_begin = key_begin;
  t->key_end = key_end;
  auto fail = [&](hipError_t e, const char* what) {
    const int rc = hip_fail(e, what, __FILE__, __LINE__);
    psg_table_destroy(t);
    return rc;
  };
  hipError_t e;
  if ((e = hipHostMalloc((void**)&t->flags_host, kNFlags * sizeof(int),
                         hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
    return fail(e, "hipHostMalloc(flags)");
  if ((e = hipHostGetDevicePointer((void**)&t->flags, t->flags_host, 0)) != hipSuccess)
    return fail(e, "hipHostGetDevicePointer(flags)");
  if (capacity > 0) {
    if ((e = hipMalloc((void**)&t->keys, capacity * sizeof(uint64_t))) != hipSuccess)
      return fail(e, "hipMalloc(table keys)");
    if ((e = hipMalloc(&t->rows, capacity * (uint64_t)width * es)) != hipSuccess)
      return fail(e, "hipMalloc(table rows)");
    t->capacity = capacity;
  }
  *out = t;
  return PSG_OK;
}

int psg_table_destroy(psg_table* t) {
  if (!t) return PSG_OK;
  if (t->rows) (void)hipFree(t->rows);
  if (t->keys) (void)hipFree(t->keys);
  if (t->slots) (void)hipFree(t->slots);
  if (t->mom) (void)hipFree(t->mom);
  if (t->any_buf) (void)hipFree(t->any_buf);
  if (t->gate) (void)hipFree(t->gate);
  if (t->flags_host) (void)hipHostFree(t->flags_host);
  delete t;
  return PSG_OK;
}

int psg_table_get_info(psg_table* t, psg_table_info* info) {
  PSG_REQUIRE(t && info, PSG_ERR_INVALID, "psg_table_get_info: null argument");
  info->dtype = t->dtype;
  info->width = t->width;
  info->key_begin = t->key_begin;
  info->key_end = t->key_end;
  info->size = t->size;
  info->capacity = t->capacity;
  info->rows = t->rows;
  info->keys = t->keys;
  return PSG_OK;
}

int psg_table_clear(psg_table* t, psg_stream stream) {
  PSG_REQUIRE(t, PSG_ERR_INVALID, "psg_table_clear: null table");
  (void)stream;  // every request has completed when its call returned: nothing to order behind
  t->size = 0;
  return PSG_OK;
}

int psg_table_handle(psg_table* t, int flags, const uint64_t* keys, const void* vals, void* out, uint64_t n,
                     psg_stream stream) {
  return serve("psg_table_handle", false, false, t, flags, keys, vals, out, n, 0.f, 0, stream);
}

int psg_table_handle_any(psg_table* t, int flags, const uint64_t* keys, const void* vals, void* out, uint64_t n,
                         psg_stream stream) {
  return serve("psg_table_handle_any", false, true, t, flags, keys, vals, out, n, 0.f, 0, stream);
}

int psg_table_dump(psg_table* t, uint64_t* keys_host, void* rows_host) {
  PSG_REQUIRE(t && rows_host, PSG_ERR_INVALID, "psg_table_dump: null argument");
  PSG_HIP(hipDeviceSynchronize());
  if (t->size == 0) return PSG_OK;
  PSG_HIP(hipMemcpy(rows_host, t->rows, t->size * (uint64_t)t->width * t->esize, hipMemcpyDeviceToHost));
  if (keys_host) PSG_HIP(hipMemcpy(keys_host, t->keys, t->size * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return PSG_OK;
}

int psg_table_set_adam(psg_table* t, double learning_rate, double beta1, double beta2, double epsilon) {
  PSG_REQUIRE(t, PSG_ERR_INVALID, "psg_table_set_adam: null table");
  PSG_REQUIRE(t->dtype == PSG_F32, PSG_ERR_UNSUPPORTED, "psg_table_set_adam: the update is built for F32 tables");
  PSG_REQUIRE(!t->adam, PSG_ERR_INVALID, "psg_table_set_adam: the table already has Adam state");
  PSG_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1, PSG_ERR_INVALID,
              "psg_table_set_adam: beta1 %g / beta2 %g outside [0, 1)", beta1, beta2);
  PSG_REQUIRE(epsilon >= 0, PSG_ERR_INVALID, "psg_table_set_adam: epsilon %g below 0", epsilon);
  if (t->capacity) {
    double* mom = nullptr;
    PSG_HIP(hipMalloc((void**)&mom, t->capacity * mom_row_bytes(t)));
    // null-stream memset, waited for: done before the caller's streams use the moments
    hipError_t e = t->size ? hipMemset(mom, 0, t->size * mom_row_bytes(t)) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
      (void)hipFree(mom);
      return hip_fail(e, "psg_table_set_adam", __FILE__, __LINE__);
    }
    t->mom = mom;
  }
  t->adam = 1;
  t->alr = learning_rate;
  t->beta1 = beta1;
  t->beta2 = beta2;
  t->eps = epsilon;
  return PSG_OK;
}

int psg_table_update(psg_table* t, int flags, const uint64_t* keys, const float* grads, float* out, uint64_t n,
                     float lr, int iteration, psg_stream stream) {
  return serve("psg_table_update", true, false, t, flags, keys, grads, out, n, lr, iteration, stream);
}

int psg_table_update_any(psg_table* t, int flags, const uint64_t* keys, const float* grads, float* out, uint64_t n,
                         float lr, int iteration, psg_stream stream) {
  return serve("psg_table_update_any", true, true, t, flags, keys, grads, out, n, lr, iteration, stream);
}

// ---- the merged update ------------------------------------------------------------
int psg_table_update_merged(psg_table* t, int flags, int k, const uint64_t* const* keys, const uint64_t* ns,
                            const float* const* grads, float* const* outs, float lr, int iteration, psg_stream stream,
                            int* path_host) {
  const char* name = "psg_table_update_merged";
  PSG_TRY(require_table(name, t));
  PSG_TRY(require_frame_count(name, k));
  PSG_TRY(require_update_flags(name, flags));
  PSG_TRY(require_iteration(name, iteration));
  PSG_REQUIRE(keys && ns && grads, PSG_ERR_INVALID, "%s: null keys, ns or grads array", name);
  PSG_REQUIRE(!(flags & PSG_PULL) || outs, PSG_ERR_INVALID, "%s: pull without outs array", name);
  const bool pull = (flags & PSG_PULL) != 0;
  Frames f = round_frames(k);
  uint64_t N = 0;
  bool same = true;
  bool vec = t->width % 4 == 0;
  for (int j = 0; j < k; ++j) {
    PSG_TRY(require_round_count(name, N, ns[j]));
    f.off[j] = (uint32_t)N;
    N += ns[j];
    same = same && ns[j] == ns[0];
    if (ns[j] == 0) continue;
    PSG_REQUIRE(keys[j] && grads[j], PSG_ERR_INVALID, "%s: null keys or grads of frame %d", name, j);
    PSG_REQUIRE(!pull || outs[j], PSG_ERR_INVALID, "%s: pull without out buffer of frame %d", name, j);
    f.vals[j] = grads[j];
    f.out[j] = pull ? outs[j] : nullptr;
    vec = vec && aligned16(grads[j]) && (!pull || aligned16(outs[j]));  // optimize_vec's condition, every frame
  }
  PSG_TRY(require_f32(name, t));
  if (path_host) *path_host = 0;
  if (N == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  // the same-list round: equal counts, list 0 strictly ascending, every list equal to it
  const uint64_t n = ns[0];
  if (same && k > 1) {
    // the head of the lists first, one block: shuffled or differing lists are
    // told apart here, for one small launch instead of a resolve of list 0
    memset(t->flags_host, 0, kNFlags * sizeof(int));
    PSG_TRY(keys_differ(t, k, keys, std::min<uint64_t>(n, kRowTile), true, st));
    same = !t->flags_host[R_DIFFER];
  }
  bool resolved = false;  // t->flags_host holds the flags of the whole round's keys
  if (same) {
    PSG_TRY(resolve_first(t, keys[0], n, true, st));
    resolved = k == 1;  // list 0 is the concatenation
    same = !t->flags_host[R_UNSORTED];
  }
  if (same) {
    PSG_TRY(require_in_range(t));
    PSG_TRY(keys_differ(t, k, keys, n, false, st));
    same = !t->flags_host[R_DIFFER];
  }
  AnyPlan plan;
  const AnyPlan* p = nullptr;
  if (same) {
    PSG_TRY(resolve_finish(t, keys[0], n, st));
  } else {
    // the k lists one behind the other in the sort's key buffer; every key is
    // checked against the range before the sort (and before the first write)
    AnyScratch a;
    PSG_TRY(any_scratch(t, N, &a));
    for (int j = 0; j < k; ++j) PSG_TRY(copy_keys(a, f.off[j], keys[j], ns[j], st));
    if (!resolved) PSG_TRY(resolve_first(t, a.k0, N, true, st));
    PSG_TRY(require_in_range(t));
    PSG_TRY(plan_scratch(t, a, N, &plan, st));
    p = &plan;
    // a position of the concatenation indexes a frame's arrays moved back by its offset
    for (int j = 0; j < k; ++j) {
      if (f.vals[j]) f.vals[j] = moved_back(t, f.vals[j], f.off[j]);
      if (f.out[j]) f.out[j] = moved_back(t, f.out[j], f.off[j]);
    }
  }
  PSG_TRY(with_opt_unit(t, vec, lr, iteration, [&](auto unit, uint32_t upr, const auto& prm) {
    using UNIT = typename decltype(unit)::type;
    return flags == PSG_PUSH ? launch_merged<UNIT, PSG_PUSH>(t, p, f, n, upr, prm, st)
                             : launch_merged<UNIT, PSG_PUSH | PSG_PULL>(t, p, f, n, upr, prm, st);
  }));
  // complete on return: keys and grads no longer read, the replies in memory
  PSG_HIP(hipStreamSynchronize(st));
  if (path_host) *path_host = same ? PSG_MERGED_SAME_LIST : PSG_MERGED_SORTED;
  return PSG_OK;
}

// ---- the initial rows ---------------------------------------------------------------
int psg_table_set_init(psg_table* t, int kind, uint64_t seed, float lo, float hi) {
  const char* name = "psg_table_set_init";
  PSG_TRY(require_table(name, t));
  PSG_REQUIRE(kind == PSG_INIT_ZERO || kind == PSG_INIT_UNIFORM, PSG_ERR_INVALID, "%s: kind %d is no initializer", name,
              kind);
  PSG_REQUIRE(!t->init_set, PSG_ERR_INVALID, "%s: the table already has an initializer", name);
  PSG_TRY(require_uniform(name, lo, hi));
  t->init_set = 1;
  t->init_kind = kind;
  t->init_seed = seed;
  t->init_lo = lo;
  t->init_hi = hi;
  return PSG_OK;
}

int psg_table_get_init(psg_table* t, int* kind, uint64_t* seed, float* lo, float* hi) {
  PSG_REQUIRE(t && kind, PSG_ERR_INVALID, "psg_table_get_init: null argument");
  *kind = t->init_kind;
  if (seed) *seed = t->init_seed;
  if (lo) *lo = t->init_lo;
  if (hi) *hi = t->init_hi;
  return PSG_OK;
}

int psg_init_rows(void* out, const uint64_t* keys, uint64_t n, int dtype, uint32_t width, uint64_t seed, float lo,
                  float hi, psg_stream stream) {
  const char* name = "psg_init_rows";
  const int es = dtype_size(dtype);
  PSG_REQUIRE(es > 0, PSG_ERR_INVALID, "%s: bad dtype %d", name, dtype);
  PSG_REQUIRE(width >= 1 && width <= 4096, PSG_ERR_INVALID, "%s: width %u outside [1, 4096]", name, width);
  PSG_REQUIRE(out || n == 0, PSG_ERR_INVALID, "%s: null out", name);
  PSG_REQUIRE(keys || n == 0, PSG_ERR_INVALID, "%s: null keys", name);
  PSG_REQUIRE((reinterpret_cast<uintptr_t>(out) & (uintptr_t)(es - 1)) == 0, PSG_ERR_INVALID,
              "%s: out not on an element boundary", name);
  PSG_TRY(require_uniform(name, lo, hi));
  PSG_TRY(require_count(name, n));
  if (n == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = ((uint64_t)width * es) % 16 == 0 && aligned16(out);
  PSG_TRY(launch_init(dtype, width, out, keys, nullptr, n, vec, init_spec(seed, lo, hi), st));
  // complete on return: keys no longer read, out in memory
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

int psg_table_get_adam(psg_table* t, int* has_adam, double* params4) {
  PSG_REQUIRE(t && has_adam, PSG_ERR_INVALID, "psg_table_get_adam: null argument");
  *has_adam = t->adam;
  if (params4) params4[0] = t->alr, params4[1] = t->beta1, params4[2] = t->beta2, params4[3] = t->eps;
  return PSG_OK;
}

// ---- assign and export ------------------------------------------------------------
int psg_table_assign(psg_table* t, const uint64_t* keys, const void* rows, const double* m, const double* v,
                     uint64_t n, psg_stream stream) {
  const char* name = "psg_table_assign";
  PSG_TRY(require_table(name, t));
  PSG_REQUIRE((m != nullptr) == (v != nullptr), PSG_ERR_INVALID, "%s: m and v come as a pair, %s is null", name,
              m ? "v" : "m");
  PSG_REQUIRE(!m || t->adam, PSG_ERR_INVALID, "%s: moments for a table without Adam state", name);
  if (n == 0) return PSG_OK;
  PSG_TRY(require_keys(name, keys));
  PSG_REQUIRE(rows || !m, PSG_ERR_INVALID, "%s: moments without rows", name);
  PSG_TRY(require_count(name, n));
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(resolve_request(t, keys, n, st));
  // no rows: the list's absent keys are in the table now (one merge for a whole
  // model, where assigning it chunk by chunk would merge once per chunk)
  if (!rows) return PSG_OK;
  const uint32_t row_bytes = t->width * (uint32_t)t->esize;
  PSG_TRY(for_raw_unit(request_unit_bytes(t, PSG_PUSH, rows, nullptr), [&](auto u) {
    return launch_set<decltype(u)>(t, rows, n, row_bytes / (uint32_t)sizeof(u), st);
  }));
  if (m) PSG_TRY(move_moments<true>(t, t->slots, 0, m, v, n, st));
  // complete on return: keys, rows, m and v are no longer read
  PSG_HIP(hipStreamSynchronize(st));
  return PSG_OK;
}

int psg_table_export(psg_table* t, uint64_t first, uint64_t count, uint64_t* keys_out, void* rows_out,
                     double* m_out, double* v_out, psg_stream stream) {
  const char* name = "psg_table_export";
  PSG_TRY(require_table(name, t));
  PSG_REQUIRE((m_out != nullptr) == (v_out != nullptr), PSG_ERR_INVALID, "%s: m_out and v_out come as a pair, %s is null",
              name, m_out ? "v_out" : "m_out");
  PSG_REQUIRE(!m_out || t->adam, PSG_ERR_INVALID, "%s: moments of a table without Adam state", name);
  PSG_REQUIRE(first <= t->size && count <= t->size - first, PSG_ERR_INVALID,
              "%s: rows [%llu, %llu + %llu) of a table of %llu", name, (unsigned long long)first,
              (unsigned long long)first, (unsigned long long)count, (unsigned long long)t->size);
  if (count == 0) return PSG_OK;
  PSG_REQUIRE(rows_out, PSG_ERR_INVALID, "%s: null rows_out", name);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t row_bytes = (uint64_t)t->width * t->esize;
  // keys and rows are in key order in the table: two copies inside HBM
  if (keys_out)
    PSG_HIP(hipMemcpyAsync(keys_out, t->keys + first, count * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  PSG_HIP(hipMemcpyAsync(rows_out, (const char*)t->rows + first * row_bytes, count * row_bytes,
                         hipMemcpyDeviceToDevice, st));
  if (m_out) PSG_TRY(move_moments<false>(t, nullptr, first, m_out, v_out, count, st));
  return PSG_OK;
}

// ---- lookup and erase: the calls that never insert ---------------------------------
int psg_table_lookup(psg_table* t, const uint64_t* keys, void* out, uint8_t* found, uint64_t n, psg_stream stream) {
  const char* name = "psg_table_lookup";
  PSG_TRY(require_table(name, t));
  if (n == 0) return PSG_OK;
  PSG_TRY(require_keys(name, keys));
  PSG_REQUIRE(out || found, PSG_ERR_INVALID, "%s: out and found are both null", name);
  PSG_TRY(require_count(name, n));
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(gate_begin(t, n, st));
  PSG_TRY(launch_resolve(t, keys, n, t->gate, false, st));
  // presence alone (out null) has no unit: it is launched as one 16-B unit a row
  const uint32_t row_bytes = out ? t->width * (uint32_t)t->esize : 16;
  if (has_init(t) && out) {  // presence alone is the same with and without an initializer
    const bool vec = accumulate_vec(t, PSG_PULL, nullptr, out);
    PSG_TRY(with_dtype(t->dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (vec) return launch_read_init<DT, true>(t, keys, out, found, n, t->width / Elem<DT>::kVec, st);
      return launch_read_init<DT, false>(t, keys, out, found, n, t->width, st);
    }));
  } else {
    PSG_TRY(for_raw_unit(out ? request_unit_bytes(t, PSG_PULL, nullptr, out) : 16, [&](auto u) {
      return launch_read<decltype(u)>(t, out, found, n, row_bytes / (uint32_t)sizeof(u), st);
    }));
  }
  // the one synchronisation: keys no longer read, the reply in memory, the flags on the host
  PSG_TRY(gate_end(t, st));
  return require_in_range(t);
}

// insert_missing backwards: the slots the list names are marked dead, the
// ordered compaction over the S slots gives the survivors' old slots, and keys,
// rows and moment rows are gathered into new arrays that replace the old ones
// after one synchronisation.
int psg_table_erase(psg_table* t, const uint64_t* keys, uint64_t n, uint64_t* erased_host, psg_stream stream) {
  const char* name = "psg_table_erase";
  PSG_TRY(require_table(name, t));
  if (erased_host) *erased_host = 0;
  if (n == 0) return PSG_OK;
  PSG_TRY(require_keys(name, keys));
  PSG_TRY(require_count(name, n));
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(resolve_first(t, keys, n, false, st));
  PSG_TRY(require_in_range(t));
  const uint64_t S = t->size;
  if (S == 0) return PSG_OK;
  const uint64_t ntiles = compact_tiles(S);
  DevBuf dead, counts, from;
  PSG_HIP(hipMalloc(&dead.p, S));
  PSG_HIP(hipMalloc(&counts.p, (ntiles + 1) * sizeof(uint32_t)));
  PSG_HIP(hipMemsetAsync(dead.p, 0, S, st));
  k_mark_dead<<<grid_per_lane(n), kBlock, 0, st>>>(t->slots, n, (uint8_t*)dead.p);
  const Alive alive = {(const uint8_t*)dead.p};
  compact_count(S, (uint32_t*)counts.p, alive, st);
  PSG_HIP(hipGetLastError());
  uint64_t m = 0;  // the survivors
  PSG_TRY(read_count((const uint32_t*)counts.p + ntiles, &m, st));
  PSG_REQUIRE(m <= S, PSG_ERR_HIP, "%s: %llu survivors of %llu rows", name, (unsigned long long)m, (unsigned long long)S);
  if (m == S) return PSG_OK;  // no key of the list is present
  DevBuf K2, R2, M2;
  uint64_t cap = 0;
  if (m) {
    cap = std::max<uint64_t>(m, 1024);
    const uint64_t row_bytes = (uint64_t)t->width * t->esize;
    PSG_HIP(hipMalloc(&from.p, m * sizeof(uint32_t)));
    PSG_HIP(hipMalloc(&K2.p, cap * sizeof(uint64_t)));
    PSG_HIP(hipMalloc(&R2.p, cap * row_bytes));
    if (t->adam) PSG_HIP(hipMalloc(&M2.p, cap * mom_row_bytes(t)));
    compact_emit(S, (const uint32_t*)counts.p, alive, EmitSurvivor{t->keys, (uint64_t*)K2.p, (uint32_t*)from.p}, st);
    PSG_HIP(hipGetLastError());
    PSG_TRY(move_rows(t, true, t->rows, R2.p, (const uint32_t*)from.p, m, st));
    if (t->adam) PSG_TRY(launch_move<u32x4>(true, t->mom, M2.p, (const uint32_t*)from.p, m, t->width, st));
    PSG_HIP(hipStreamSynchronize(st));
  }
  // a table whose last key went keeps no arrays
  publish_arrays(t, K2, R2, M2, m, cap);
  if (erased_host) *erased_host = S - m;
  return PSG_OK;
}

// ---- the pooled calls ---------------------------------------------------------------
int psg_table_lookup_pooled(psg_table* t, const uint64_t* keys, const uint64_t* offsets, void* out, uint64_t n,
                            uint64_t nb, psg_stream stream) {
  return lookup_pooled("psg_table_lookup_pooled", t, keys, offsets, nullptr, PSG_POOL_SUM, out, n, nb, stream);
}

int psg_table_lookup_pooled_weighted(psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* weights,
                                     int mode, void* out, uint64_t n, uint64_t nb, psg_stream stream) {
  return lookup_pooled("psg_table_lookup_pooled_weighted", t, keys, offsets, weights, mode, out, n, nb, stream);
}

int psg_table_update_pooled(psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* grads,
                            uint64_t n, uint64_t nb, float lr, int iteration, psg_stream stream) {
  return update_pooled("psg_table_update_pooled", t, keys, offsets, nullptr, PSG_POOL_SUM, grads, n, nb, lr, iteration,
                       stream, nullptr);
}

int psg_table_update_pooled_weighted(psg_table* t, const uint64_t* keys, const uint64_t* offsets, const float* weights,
                                     int mode, const float* grads, uint64_t n, uint64_t nb, float lr, int iteration,
                                     psg_stream stream) {
  return update_pooled("psg_table_update_pooled_weighted", t, keys, offsets, weights, mode, grads, n, nb, lr, iteration,
                       stream, nullptr);
}

// ---- the round of pooled and plain frames ------------------------------------------
// psg_table_update_merged's sorted path with update_pooled's payload: the k key
// lists one behind the other in the sort's key buffer and, in its payload
// buffer, every occurrence's gradient row in the frames' gradient arrays laid
// end to end (k_row_index for a plain frame, k_bag_of for a pooled one, each
// from its frame's first row).  A round of plain frames is
// psg_table_update_merged's, one pooled frame is update_pooled's.
int psg_table_update_pooled_merged(psg_table* t, int k, const uint64_t* const* keys, const uint64_t* ns,
                                   const uint64_t* const* offsets, const uint64_t* nbs, const float* const* grads,
                                   float lr, int iteration, psg_stream stream, int* path_host) {
  const char* name = "psg_table_update_pooled_merged";
  PSG_TRY(require_table(name, t));
  PSG_TRY(require_frame_count(name, k));
  PSG_TRY(require_iteration(name, iteration));
  PSG_REQUIRE(keys && ns && offsets && nbs && grads, PSG_ERR_INVALID, "%s: null keys, ns, offsets, nbs or grads array",
              name);
  bool pooled = false;
  for (int j = 0; j < k; ++j) {
    PSG_REQUIRE(keys[j] || ns[j] == 0, PSG_ERR_INVALID, "%s: null keys of frame %d", name, j);
    if (offsets[j]) {
      pooled = true;
      PSG_REQUIRE(grads[j] || nbs[j] == 0, PSG_ERR_INVALID, "%s: null grads of pooled frame %d", name, j);
      PSG_REQUIRE(nbs[j] > 0 || ns[j] == 0, PSG_ERR_INVALID, "%s: %llu keys of frame %d and no bag to hold them", name,
                  (unsigned long long)ns[j], j);
    } else {
      PSG_REQUIRE(grads[j] || ns[j] == 0, PSG_ERR_INVALID, "%s: null grads of frame %d", name, j);
    }
  }
  Frames f = round_frames(k);  // off: the first gradient row of each frame
  decltype(f.off) koff;         // the first key of each frame in the concatenation
  uint64_t N = 0, G = 0;
  for (int j = 0; j < k; ++j) {
    const uint64_t g = offsets[j] ? nbs[j] : ns[j];
    PSG_TRY(require_round_count(name, N, ns[j]));
    PSG_TRY(require_round_count(name, G, g, "gradient rows"));
    koff[j] = (uint32_t)N;
    f.off[j] = (uint32_t)G;
    N += ns[j];
    G += g;
  }
  PSG_TRY(require_f32(name, t));
  if (path_host) *path_host = 0;
  if (!pooled) return psg_table_update_merged(t, PSG_PUSH, k, keys, ns, grads, nullptr, lr, iteration, stream, path_host);
  if (k == 1)
    return update_pooled(name, t, keys[0], offsets[0], nullptr, PSG_POOL_SUM, grads[0], ns[0], nbs[0], lr, iteration,
                         stream, path_host);
  if (N == 0 && G == 0) return PSG_OK;  // no key and no bag: nothing to check either
  hipStream_t st = (hipStream_t)stream;
  // the front half: every offsets array checked before anything else reads it,
  // every key against the range; one synchronisation, nothing written yet
  AnyScratch a = {};
  if (N) {
    PSG_TRY(ensure_slots(t, N));  // ahead of resolve_first's own: the slots grow before the sort's scratch, as ever
    PSG_TRY(any_scratch(t, N, &a));
  }
  PSG_TRY(resolve_first(t, a.k0, N, true, st, [&] {
    for (int j = 0; j < k; ++j) {
      if (offsets[j] && nbs[j]) PSG_TRY(launch_offsets_check(offsets[j], ns[j], nbs[j], t->flags, st));
      PSG_TRY(copy_keys(a, koff[j], keys[j], ns[j], st));
    }
    return (int)PSG_OK;
  }));
  PSG_REQUIRE(!t->flags_host[R_OFFSETS], PSG_ERR_INVALID,
              "%s: the offsets of a pooled frame do not start at 0, ascend and end at its ns", name);
  PSG_TRY(require_in_range(t));
  if (N == 0) return PSG_OK;  // every frame is empty: no gradient row is read
  // the payload, and each frame's array moved back by its first row; 16-B units
  // under optimize_vec's condition on every array that is read
  bool vec = t->width % 4 == 0;
  for (int j = 0; j < k; ++j) {
    if (ns[j] == 0) continue;
    if (offsets[j])
      k_bag_of<<<grid_per_lane(nbs[j]), kBlock, 0, st>>>(offsets[j], nbs[j], f.off[j], a.p0 + koff[j]);
    else
      k_row_index<<<grid_per_lane(ns[j]), kBlock, 0, st>>>(a.p0 + koff[j], ns[j], f.off[j]);
    PSG_HIP(hipGetLastError());
    vec = vec && aligned16(grads[j]);
    f.vals[j] = moved_back(t, (const void*)grads[j], f.off[j]);
  }
  AnyPlan plan;
  PSG_TRY(plan_scratch(t, a, N, &plan, st, true));
  PSG_TRY(pooled_step(t, vec, &plan, nullptr, nullptr, &f, {}, N, lr, iteration, st));
  // complete on return: keys, offsets and grads no longer read
  PSG_HIP(hipStreamSynchronize(st));
  if (path_host) *path_host = PSG_MERGED_SORTED;
  return PSG_OK;
}

int psg_table_dump_moments(psg_table* t, double* m_host, double* v_host) {
  PSG_REQUIRE(t, PSG_ERR_INVALID, "psg_table_dump_moments: null table");
  PSG_REQUIRE(t->adam, PSG_ERR_INVALID, "psg_table_dump_moments: the table has no Adam state");
  if (t->size == 0) return PSG_OK;
  PSG_REQUIRE(m_host && v_host, PSG_ERR_INVALID, "psg_table_dump_moments: null argument");
  PSG_HIP(hipDeviceSynchronize());
  const uint64_t W = t->width;
  std::vector<double> raw(t->size * 2 * W);
  PSG_HIP(hipMemcpy(raw.data(), t->mom, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (uint64_t r = 0; r < t->size; ++r)
    for (uint32_t j = 0; j < W; ++j) {
      const uint32_t c = mom_col(j, t->width);
      m_host[r * W + j] = raw[r * 2 * W + c];
      v_host[r * W + j] = raw[r * 2 * W + W + c];
    }
  return PSG_OK;
}

}  // extern "C"
