// psg_qrows.hip — the frozen 8-bit row-wise snapshot of a row table (psg_qtable_*,
// psg_table_freeze_q8; include/psg.h has the definition of a frozen row and
// DESIGN.md §3.5.16 the layouts and the numbers).  The reference has no such
// object: its server keeps f32 values and nothing smaller.
//
// A snapshot is K[S] (the table's keys, ascending) and Q[S * stride] bytes, row s
// at Q + s * stride with stride = round_up(round_up(W, 4) + 8, 16):
//   bytes [0, W)            one code per column
//   bytes [W, hdr)          zero, hdr = round_up(W, 4)
//   bytes [hdr, hdr + 8)    scale, bias: two f32
//   bytes [hdr + 8, stride) zero
// so every row starts on 16 B, unit u of a row is columns 16u .. 16u + 15 and a
// 16-B load of the last unit stays inside the row (16 * ceil(W / 16) <= stride).
//
// Two kernels carry it.  k_qrows_freeze makes rows: a group of lanes owns a source
// row in registers (k_rows_walk_rowwise's ownership), reduces min and max over the
// group by a shuffle butterfly, and every lane encodes and stores its own columns.
// k_qrows_pool reads them: (bag, unit) pairs in k_rows_pool's flat order behind
// the same gate word, a unit 16 codes in one 16-B load widened into 16 f32 sums.
// The front half of a request — the any-order resolve, the offsets check — is the
// row table's own (rows_resolve_any / rows_offsets_check, psg_rows.hip), unchanged.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "psg_internal.h"

struct psg_qtable {
  uint32_t width;
  uint32_t stride;  // bytes a row
  uint32_t hdr;     // where scale and bias stand in a row
  uint64_t key_begin, key_end;
  uint64_t size;
  uint64_t* keys;  // device, size
  uint8_t* rows;   // device, size * stride
  // request scratch, the snapshot's own: slots (grown on demand), the lookups' flag
  // words on the device, and the pinned words the host reads (kernels write `flags`,
  // the device's view of flags_host)
  uint32_t* slots;
  uint64_t slots_cap;
  int* gate;
  int* flags;
  int* flags_host;
};

namespace psg {
namespace {

constexpr uint64_t kMaxRows = 0xfffffffeull;
enum { Q_REFUSED = 0, Q_UNSORTED = 2 };  // flag words beside kRowFlagRange / kRowFlagOffsets

__device__ __forceinline__ void raise(int* flags, int which, bool cond) {
  if (__ballot(cond) && (threadIdx.x & 63) == 0) flags[which] = 1;
}

unsigned grid_for(uint64_t blocks) {
  const uint64_t cap = (uint64_t)max_stream_blocks();
  if (blocks > cap) blocks = cap;
  return blocks ? (unsigned)blocks : 1u;
}

inline uint32_t q_hdr(uint32_t W) { return (W + 3u) & ~3u; }
inline uint32_t q_stride(uint32_t W) { return (q_hdr(W) + 8u + 15u) & ~15u; }

// ---- freeze ---------------------------------------------------------------------------
// min and max that put -0.0 below +0.0, so lo, hi and with them `range` and `scale`
// are the same bits in whatever order the columns meet.  A NaN loses every
// comparison and is caught by the finiteness test beside them.
__device__ __forceinline__ float min_z(float a, float b) { return (b < a || (b == a && signbit(b))) ? b : a; }
__device__ __forceinline__ float max_z(float a, float b) { return (b > a || (b == a && !signbit(b))) ? b : a; }

// One code: the column's distance from lo in steps of scale, a correctly rounded
// division, to the nearest even integer, clamped (the quotient can reach 255.00002).
__device__ __forceinline__ uint32_t q_code(float x, float lo, float scale) {
  return scale == 0.0f ? 0u : (uint32_t)fminf(rintf((x - lo) / scale), 255.0f);
}

// A GROUP of G = 2^lg lanes (G <= 64: inside one wave) owns source row s = slot s;
// lane l holds its units l, l + G, ... as f32, UPL of them (a compile-time bound:
// the row lives in registers, no LDS, no scratch).  A unit is 16 B of the source
// (VEC: E = 4 f32 or 8 half columns) or one element.  Pass 1 is in-lane: lo, hi and
// a finiteness bit over the lane's columns.  Then a butterfly over the group,
// x = op(x, shfl_xor(x, d)) for d = G/2 .. 1: min_z and max_z are exact and
// commute, so every lane ends with the row's lo and hi; range, scale, bias and the
// refusal are then uniform across the group and computed by every lane.  Pass 2 is
// in-lane again: a lane encodes its own columns and stores them packed — an f32
// unit is one 32-bit word of four codes, a half unit 8 B of eight, an element one
// byte — and lane 0 stores the header.  The source is read once, the row written
// once, one writer per byte.  The padding bytes are the host's (the array is
// cleared when it is made).  A refused row (a NaN or an infinity in it, or a range
// that is not finite) stores nothing and raises Q_REFUSED.
// The row loop is uniform over the block: a group past the last row takes every
// shuffle its neighbours take, on +inf / -inf, and stores nothing.
template <int DT, bool VEC, int UPL>
__global__ __launch_bounds__(256) void k_qrows_freeze(const typename PoolAcc<DT, VEC>::U* __restrict__ R,
                                                      uint8_t* __restrict__ Q, uint64_t S, uint32_t upr, uint32_t lg,
                                                      uint32_t stride, uint32_t hdr, int* __restrict__ flags) {
  using ACC = PoolAcc<DT, VEC>;
  constexpr int E = VEC ? Elem<DT>::kVec : 1;
  const uint32_t G = 1u << lg;
  const uint32_t l = threadIdx.x & (G - 1);
  const uint32_t gpb = (uint32_t)kBlock >> lg;  // groups, and rows at a time, per block
  const uint64_t step = (uint64_t)gridDim.x * gpb;
  bool refused = false;
  for (uint64_t base = (uint64_t)blockIdx.x * gpb; base < S; base += step) {
    const uint64_t s = base + (threadIdx.x >> lg);
    const bool row = s < S;
    float x[UPL][E];
    float lo = INFINITY, hi = -INFINITY;
    int wild = 0;
#pragma unroll
    for (int k = 0; k < UPL; ++k) {
      const uint32_t c = l + (uint32_t)k * G;
      const bool in = row && c < upr;
      typename ACC::A a = {};
      if (in) a = ACC::widen(R[s * upr + c]);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if constexpr (VEC) x[k][e] = a[e];
        else x[k][e] = a;
        if (in) {
          lo = min_z(lo, x[k][e]);
          hi = max_z(hi, x[k][e]);
          wild |= !(fabsf(x[k][e]) <= FLT_MAX);
        }
      }
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
      if (d >= G) continue;
      lo = min_z(lo, __shfl_xor(lo, (int)d, 64));
      hi = max_z(hi, __shfl_xor(hi, (int)d, 64));
      wild |= __shfl_xor(wild, (int)d, 64);
    }
    const float range = hi - lo;
    const float scale = range / 255.0f;
    const float bias = lo + 0.0f;  // a -0.0 minimum is kept as +0.0
    const bool refuse = row && (wild || !(range <= FLT_MAX));
    refused |= refuse;
    if (!row || refuse) continue;
    uint8_t* const qr = Q + s * stride;
#pragma unroll
    for (int k = 0; k < UPL; ++k) {
      const uint32_t c = l + (uint32_t)k * G;
      if (c >= upr) continue;
      if constexpr (VEC) {
        uint32_t word[E / 4];
#pragma unroll
        for (int j = 0; j < E / 4; ++j)
          word[j] = q_code(x[k][4 * j], lo, scale) | q_code(x[k][4 * j + 1], lo, scale) << 8 |
                    q_code(x[k][4 * j + 2], lo, scale) << 16 | q_code(x[k][4 * j + 3], lo, scale) << 24;
        if constexpr (E == 4) *reinterpret_cast<uint32_t*>(qr + 4 * c) = word[0];
        else *reinterpret_cast<uint2*>(qr + 8 * c) = make_uint2(word[0], word[1]);
      } else {
        qr[c] = (uint8_t)q_code(x[k][0], lo, scale);
      }
    }
    if (l == 0) {
      float* const h = reinterpret_cast<float*>(qr + hdr);
      h[0] = scale;
      h[1] = bias;
    }
  }
  raise(flags, Q_REFUSED, refused);
}

// ---- read: bags and single rows ---------------------------------------------------------
// Pass 2 of psg_qtable_lookup_pooled and psg_qtable_lookup, launched behind the
// offsets check and the resolve WITHOUT the host in between, as k_rows_pool is: a
// launch that finds R_RANGE or R_OFFSETS raised in `gate` returns before it has
// read one offset.  Lanes take (bag, unit) pairs in RowWalk's flat order; a unit is
// the u32x4 at row + 16 * unit: 16 codes, widened into 16 f32 accumulators that
// start from +0.  Per position the slot (and the weight, kQWeighted) is loaded two
// ahead; the row's unit and its 8-B header one ahead, the two loads issued together
// and both addresses made from the slot alone.  A code is read back as
// x = (float)code * scale + bias, one multiply and then one add (the file is built
// with -ffp-contract=off), and enters the sum as an f32 row's column does in
// k_rows_pool: acc + x, or acc + w * x, one rounding each; kQMean divides the sum
// once by the bag's whole length.  An absent slot loads nothing and adds nothing.
// One writer per output column, no atomics, no LDS: VEC_OUT (out on 16 B, W % 4 ==
// 0) stores up to four f32x4, else scalar stores masked to W.
// kQRead is psg_qtable_lookup: "bag" b is position b alone, and the lane of unit 0
// writes found[b]; with out null it is presence only, one lane per position.
enum { kQSum = 0, kQWeighted = 1, kQMean = 2, kQRead = 3 };
struct QHead {
  float scale, bias;
};

template <int POOL, bool VEC_OUT>
__global__ __launch_bounds__(256) void k_qrows_pool(const uint8_t* __restrict__ Q, const uint32_t* __restrict__ slots,
                                                    const uint64_t* __restrict__ offsets,
                                                    const float* __restrict__ weights, float* __restrict__ out,
                                                    uint8_t* __restrict__ found, uint64_t nb, uint32_t W, uint32_t upr,
                                                    uint32_t rpt, uint32_t stride, uint32_t hdr,
                                                    const int* __restrict__ gate) {
  if (gate[kRowFlagRange] | gate[kRowFlagOffsets]) return;
  if constexpr (POOL == kQRead) {
    if (!out) {
      for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * kBlock)
        found[i] = slots[i] != kRowAbsent ? 1 : 0;
      return;
    }
  }
  const uint64_t ntiles = (nb + rpt - 1) / rpt;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t b0 = t * rpt;
    const uint32_t nr = (uint32_t)(nb - b0 < rpt ? nb - b0 : rpt);
    const uint32_t total = nr * upr;
    RowWalk w(threadIdx.x, upr);
    for (uint32_t e = threadIdx.x; e < total; e += kBlock, w.next()) {
      const uint64_t b = b0 + w.r;
      const uint32_t c = w.c;
      uint32_t p, pe;
      if constexpr (POOL == kQRead) {
        p = (uint32_t)b, pe = p + 1;
      } else {
        p = (uint32_t)offsets[b];  // <= n <= 2^32 - 2: checked
        pe = (uint32_t)offsets[b + 1];
      }
      [[maybe_unused]] const uint32_t len = pe - p;
      float acc[16] = {};  // +0
      if (p < pe) {
        uint32_t s0 = slots[p];
        uint32_t s1 = p + 1 < pe ? slots[p + 1] : kRowAbsent;
        [[maybe_unused]] float w0 = 0, w1 = 0;
        if constexpr (POOL == kQWeighted) {
          w0 = weights[p];
          if (p + 1 < pe) w1 = weights[p + 1];
        }
        if constexpr (POOL == kQRead)
          if (found && c == 0) found[b] = s0 != kRowAbsent ? 1 : 0;
        u32x4 v = {};
        QHead h = {};
        if (s0 != kRowAbsent) {
          const uint8_t* const r = Q + (uint64_t)s0 * stride;
          v = *reinterpret_cast<const u32x4*>(r + 16 * c);
          h = *reinterpret_cast<const QHead*>(r + hdr);
        }
        for (; p < pe; ++p) {
          const uint32_t s2 = p + 2 < pe ? slots[p + 2] : kRowAbsent;
          [[maybe_unused]] float w2 = 0;
          if constexpr (POOL == kQWeighted)
            if (p + 2 < pe) w2 = weights[p + 2];
          u32x4 vn = {};
          QHead hn = {};
          if (s1 != kRowAbsent) {
            const uint8_t* const r = Q + (uint64_t)s1 * stride;
            vn = *reinterpret_cast<const u32x4*>(r + 16 * c);
            hn = *reinterpret_cast<const QHead*>(r + hdr);
          }
          if (s0 != kRowAbsent) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              const float x = (float)((v[j >> 2] >> (8 * (j & 3))) & 0xffu) * h.scale + h.bias;
              if constexpr (POOL == kQWeighted) acc[j] = acc[j] + w0 * x;
              else acc[j] = acc[j] + x;
            }
          }
          if constexpr (POOL == kQWeighted) w0 = w1, w1 = w2;
          s0 = s1, s1 = s2, v = vn, h = hn;
        }
        if constexpr (POOL == kQMean) {
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[j] = acc[j] / (float)len;
        }
      }
      const uint32_t col = 16 * c;
      float* const o = out + b * W + col;
      if constexpr (VEC_OUT) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col + 4 * j < W)
            *reinterpret_cast<f32x4*>(o + 4 * j) = f32x4{acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (col + j < W) o[j] = acc[j];
      }
    }
  }
}

// ---- the external format -----------------------------------------------------------------
// A row across the interface is W codes, scale, bias: W + 8 bytes, no padding
// (include/psg.h).  One lane per byte, both ways: the format has no alignment to use.
__global__ __launch_bounds__(256) void k_qrows_pack(const uint8_t* __restrict__ src, uint8_t* __restrict__ Q,
                                                    uint64_t n, uint32_t W, uint32_t stride, uint32_t hdr) {
  const uint64_t total = n * stride;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = i / stride;
    const uint32_t j = (uint32_t)(i - r * stride);
    const uint8_t* const s = src + r * (W + 8);
    Q[i] = j < W ? s[j] : (j >= hdr && j < hdr + 8) ? s[W + (j - hdr)] : (uint8_t)0;
  }
}
__global__ __launch_bounds__(256) void k_qrows_unpack(const uint8_t* __restrict__ Q, uint8_t* __restrict__ dst,
                                                      uint64_t first, uint64_t count, uint32_t W, uint32_t stride,
                                                      uint32_t hdr) {
  const uint32_t rb = W + 8;
  const uint64_t total = count * rb;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = i / rb;
    const uint32_t j = (uint32_t)(i - r * rb);
    dst[i] = Q[(first + r) * stride + (j < W ? j : hdr + (j - W))];
  }
}

// The keys psg_qtable_create is given: strictly ascending and inside [kb, ke).
__global__ __launch_bounds__(256) void k_qkeys_check(const uint64_t* __restrict__ K, uint64_t n, uint64_t kb,
                                                     uint64_t ke, int* __restrict__ flags) {
  int unsorted = 0, range = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t k = K[i];
    if (i > 0 && K[i - 1] >= k) unsorted = 1;
    if (k < kb || k >= ke) range = 1;
  }
  raise(flags, Q_UNSORTED, unsorted != 0);
  raise(flags, kRowFlagRange, range != 0);
}

// ---- host side ----------------------------------------------------------------------------
void q_free(psg_qtable* q) {
  if (!q) return;
  if (q->keys) (void)hipFree(q->keys);
  if (q->rows) (void)hipFree(q->rows);
  if (q->slots) (void)hipFree(q->slots);
  if (q->gate) (void)hipFree(q->gate);
  if (q->flags_host) (void)hipHostFree(q->flags_host);
  delete q;
}

struct QOwner {  // frees a snapshot that is not handed out
  psg_qtable* q = nullptr;
  ~QOwner() { q_free(q); }
};

// A snapshot of `size` rows with its arrays allocated (none for size 0), the
// padding of every row cleared, and its pinned flag words at zero.
int q_new(uint32_t width, uint64_t kb, uint64_t ke, uint64_t size, hipStream_t st, QOwner* own) {
  psg_qtable* q = new psg_qtable();  // value-initialised: every field zero
  own->q = q;
  q->width = width;
  q->hdr = q_hdr(width);
  q->stride = q_stride(width);
  q->key_begin = kb;
  q->key_end = ke;
  q->size = size;
  PSG_HIP(hipHostMalloc((void**)&q->flags_host, kRowFlags * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  PSG_HIP(hipHostGetDevicePointer((void**)&q->flags, q->flags_host, 0));
  memset(q->flags_host, 0, kRowFlags * sizeof(int));
  if (size) {
    PSG_HIP(hipMalloc((void**)&q->keys, size * sizeof(uint64_t)));
    PSG_HIP(hipMalloc((void**)&q->rows, size * q->stride));
    PSG_HIP(hipMemsetAsync(q->rows, 0, size * q->stride, st));
  }
  return PSG_OK;
}

int q_require(const char* name, const psg_qtable* q) {
  PSG_REQUIRE(q, PSG_ERR_INVALID, "%s: null snapshot", name);
  return PSG_OK;
}
int q_require_count(const char* name, uint64_t n, const char* what) {
  PSG_REQUIRE(n <= kMaxRows, PSG_ERR_RANGE, "%s: more than 2^32-2 %s in one request", name, what);
  return PSG_OK;
}

// The lookups' front half: slot scratch for n positions, the gate word cleared on
// the stream; q_gate_end brings it to the host and is the call's one synchronisation.
int q_gate_begin(psg_qtable* q, uint64_t n, hipStream_t st) {
  if (q->slots_cap < n || !q->slots) {
    if (q->slots) PSG_HIP(hipFree(q->slots));
    q->slots = nullptr;
    q->slots_cap = 0;
    const uint64_t cap = n > (1u << 16) ? n : (1u << 16);
    PSG_HIP(hipMalloc((void**)&q->slots, cap * sizeof(uint32_t)));
    q->slots_cap = cap;
  }
  if (!q->gate) PSG_HIP(hipMalloc((void**)&q->gate, kRowFlags * sizeof(int)));
  PSG_HIP(hipMemsetAsync(q->gate, 0, kRowFlags * sizeof(int), st));
  return PSG_OK;
}
int q_gate_end(psg_qtable* q, const char* name, uint64_t n, hipStream_t st) {
  PSG_HIP(hipMemcpyAsync(q->flags_host, q->gate, kRowFlags * sizeof(int), hipMemcpyDeviceToHost, st));
  PSG_HIP(hipStreamSynchronize(st));
  PSG_REQUIRE(!q->flags_host[kRowFlagOffsets], PSG_ERR_INVALID,
              "%s: offsets do not start at 0, ascend and end at n = %llu", name, (unsigned long long)n);
  PSG_REQUIRE(!q->flags_host[kRowFlagRange], PSG_ERR_RANGE, "%s: key outside the snapshot's range [%llu, %llu)", name,
              (unsigned long long)q->key_begin, (unsigned long long)q->key_end);
  return PSG_OK;
}

template <int POOL>
int launch_qpool(psg_qtable* q, const uint64_t* offsets, const float* weights, float* out, uint8_t* found,
                 uint64_t nb, hipStream_t st) {
  const uint32_t upr = (q->width + 15) / 16;
  const uint32_t rpt = rows_per_tile(upr);
  const unsigned grid = out ? grid_for((nb + rpt - 1) / rpt) : grid_for((nb + kBlock - 1) / kBlock);
  if (out && aligned16(out) && q->width % 4 == 0)
    k_qrows_pool<POOL, true><<<grid, kBlock, 0, st>>>(q->rows, q->slots, offsets, weights, out, found, nb, q->width,
                                                      upr, rpt, q->stride, q->hdr, q->gate);
  else
    k_qrows_pool<POOL, false><<<grid, kBlock, 0, st>>>(q->rows, q->slots, offsets, weights, out, found, nb, q->width,
                                                       upr, rpt, q->stride, q->hdr, q->gate);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

// k_qrows_freeze over S rows: G = the row's units rounded up to a power of two, 64
// at most; UPL the units a lane then holds, rounded up to the next instantiation
// (1, 4, then 16 f32 or 8 half units of 16 B; element units 1, 4, 16, 64).
template <int DT, bool VEC, int UPL>
void launch_freeze_as(const TableView& v, psg_qtable* q, uint32_t upr, uint32_t lg, hipStream_t st) {
  const uint32_t gpb = (uint32_t)kBlock >> lg;
  k_qrows_freeze<DT, VEC, UPL><<<grid_for((v.size + gpb - 1) / gpb), kBlock, 0, st>>>(
      (const typename PoolAcc<DT, VEC>::U*)v.rows, q->rows, v.size, upr, lg, q->stride, q->hdr, q->flags);
}
template <int DT>
int launch_freeze(const TableView& v, psg_qtable* q, hipStream_t st) {
  constexpr uint32_t es = sizeof(typename Elem<DT>::T);
  constexpr int kWide = DT == PSG_F32 ? 16 : 8;  // 16-B units a lane holds of a 4096-column row
  const bool vec = (v.width * es) % 16 == 0;
  const uint32_t upr = vec ? v.width * es / 16 : v.width;
  uint32_t lg = 0;
  while (lg < 6 && (1u << lg) < upr) ++lg;
  const uint32_t need = (upr + 63) / 64;
  if (vec) {
    if (need <= 1) launch_freeze_as<DT, true, 1>(v, q, upr, lg, st);
    else if (need <= 4) launch_freeze_as<DT, true, 4>(v, q, upr, lg, st);
    else launch_freeze_as<DT, true, kWide>(v, q, upr, lg, st);
  } else {
    if (need <= 1) launch_freeze_as<DT, false, 1>(v, q, upr, lg, st);
    else if (need <= 4) launch_freeze_as<DT, false, 4>(v, q, upr, lg, st);
    else if (need <= 16) launch_freeze_as<DT, false, 16>(v, q, upr, lg, st);
    else launch_freeze_as<DT, false, 64>(v, q, upr, lg, st);
  }
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

}  // namespace
}  // namespace psg

using namespace psg;

extern "C" {

int psg_table_freeze_q8(psg_table* t, psg_qtable** out, psg_stream stream) {
  const char* name = "psg_table_freeze_q8";
  PSG_REQUIRE(t, PSG_ERR_INVALID, "%s: null table", name);
  PSG_REQUIRE(out, PSG_ERR_INVALID, "%s: null out", name);
  const TableView v = table_view(t);
  PSG_REQUIRE(v.dtype == PSG_F32 || v.dtype == PSG_F16 || v.dtype == PSG_BF16, PSG_ERR_UNSUPPORTED,
              "%s: the freeze is built for F32, F16 and BF16 tables", name);
  hipStream_t st = (hipStream_t)stream;
  QOwner own;
  PSG_TRY(q_new(v.width, v.key_begin, v.key_end, v.size, st, &own));
  psg_qtable* q = own.q;
  if (v.size) {
    PSG_HIP(hipMemcpyAsync(q->keys, v.keys, v.size * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    if (v.dtype == PSG_F32) PSG_TRY(launch_freeze<PSG_F32>(v, q, st));
    else if (v.dtype == PSG_F16) PSG_TRY(launch_freeze<PSG_F16>(v, q, st));
    else PSG_TRY(launch_freeze<PSG_BF16>(v, q, st));
    // the one synchronisation: the source is no longer read, the refusal on the host
    PSG_HIP(hipStreamSynchronize(st));
    PSG_REQUIRE(!q->flags_host[Q_REFUSED], PSG_ERR_INVALID,
                "%s: a row holds a NaN or an infinity, or its range is not finite", name);
  }
  own.q = nullptr;
  *out = q;
  return PSG_OK;
}

int psg_qtable_create(uint32_t width, uint64_t key_begin, uint64_t key_end, const uint64_t* keys, const void* rows,
                      uint64_t n, psg_qtable** out, psg_stream stream) {
  const char* name = "psg_qtable_create";
  PSG_REQUIRE(out, PSG_ERR_INVALID, "%s: null out", name);
  PSG_REQUIRE(width >= 1 && width <= 4096, PSG_ERR_INVALID, "%s: width %u outside [1, 4096]", name, width);
  PSG_REQUIRE(key_begin < key_end, PSG_ERR_INVALID, "%s: empty key range", name);
  PSG_REQUIRE(keys || n == 0, PSG_ERR_INVALID, "%s: null keys", name);
  PSG_REQUIRE(rows || n == 0, PSG_ERR_INVALID, "%s: null rows", name);
  PSG_TRY(q_require_count(name, n, "rows"));
  hipStream_t st = (hipStream_t)stream;
  QOwner own;
  PSG_TRY(q_new(width, key_begin, key_end, n, st, &own));
  psg_qtable* q = own.q;
  if (n) {
    k_qkeys_check<<<grid_for((n + kBlock - 1) / kBlock), kBlock, 0, st>>>(keys, n, key_begin, key_end, q->flags);
    PSG_HIP(hipGetLastError());
    PSG_HIP(hipMemcpyAsync(q->keys, keys, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    k_qrows_pack<<<grid_for((n * q->stride + kBlock - 1) / kBlock), kBlock, 0, st>>>((const uint8_t*)rows, q->rows, n,
                                                                                    width, q->stride, q->hdr);
    PSG_HIP(hipGetLastError());
    // the one synchronisation: keys and rows are no longer read, the key flags on the host
    PSG_HIP(hipStreamSynchronize(st));
    PSG_REQUIRE(!q->flags_host[Q_UNSORTED], PSG_ERR_INVALID, "%s: keys are not strictly ascending", name);
    PSG_REQUIRE(!q->flags_host[kRowFlagRange], PSG_ERR_RANGE, "%s: key outside the range [%llu, %llu)", name,
                (unsigned long long)key_begin, (unsigned long long)key_end);
  }
  own.q = nullptr;
  *out = q;
  return PSG_OK;
}

int psg_qtable_destroy(psg_qtable* q) {
  q_free(q);
  return PSG_OK;
}

int psg_qtable_get_info(psg_qtable* q, psg_qtable_info* info) {
  PSG_REQUIRE(q && info, PSG_ERR_INVALID, "psg_qtable_get_info: null argument");
  info->width = q->width;
  info->row_bytes = q->width + 8;
  info->size = q->size;
  info->key_begin = q->key_begin;
  info->key_end = q->key_end;
  info->device_bytes = q->size * (sizeof(uint64_t) + q->stride) + q->slots_cap * sizeof(uint32_t) +
                       (q->gate ? kRowFlags * sizeof(int) : 0);
  return PSG_OK;
}

int psg_qtable_export(psg_qtable* q, uint64_t first, uint64_t count, uint64_t* keys_out, void* rows_out,
                      psg_stream stream) {
  const char* name = "psg_qtable_export";
  PSG_TRY(q_require(name, q));
  PSG_REQUIRE(first <= q->size && count <= q->size - first, PSG_ERR_INVALID,
              "%s: rows [%llu, %llu + %llu) of a snapshot of %llu", name, (unsigned long long)first,
              (unsigned long long)first, (unsigned long long)count, (unsigned long long)q->size);
  if (count == 0) return PSG_OK;
  PSG_REQUIRE(rows_out, PSG_ERR_INVALID, "%s: null rows_out", name);
  hipStream_t st = (hipStream_t)stream;
  if (keys_out)
    PSG_HIP(hipMemcpyAsync(keys_out, q->keys + first, count * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  k_qrows_unpack<<<grid_for((count * (q->width + 8) + kBlock - 1) / kBlock), kBlock, 0, st>>>(
      q->rows, (uint8_t*)rows_out, first, count, q->width, q->stride, q->hdr);
  PSG_HIP(hipGetLastError());
  return PSG_OK;
}

int psg_qtable_lookup(psg_qtable* q, const uint64_t* keys, float* out, uint8_t* found, uint64_t n,
                      psg_stream stream) {
  const char* name = "psg_qtable_lookup";
  PSG_TRY(q_require(name, q));
  if (n == 0) return PSG_OK;
  PSG_REQUIRE(keys, PSG_ERR_INVALID, "%s: null keys", name);
  PSG_REQUIRE(out || found, PSG_ERR_INVALID, "%s: out and found are both null", name);
  PSG_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, PSG_ERR_INVALID, "%s: out not on a 4-B boundary", name);
  PSG_TRY(q_require_count(name, n, "keys"));
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(q_gate_begin(q, n, st));
  PSG_TRY(rows_resolve_any(keys, n, q->keys, q->size, q->key_begin, q->key_end, q->slots, q->gate, st));
  PSG_TRY(launch_qpool<kQRead>(q, nullptr, nullptr, out, found, n, st));
  return q_gate_end(q, name, n, st);
}

int psg_qtable_lookup_pooled(psg_qtable* q, const uint64_t* keys, const uint64_t* offsets, const float* weights,
                             int mode, float* out, uint64_t n, uint64_t nb, psg_stream stream) {
  const char* name = "psg_qtable_lookup_pooled";
  PSG_TRY(q_require(name, q));
  PSG_REQUIRE(keys || n == 0, PSG_ERR_INVALID, "%s: null keys", name);
  PSG_REQUIRE(offsets || nb == 0, PSG_ERR_INVALID, "%s: null offsets", name);
  PSG_REQUIRE(out || nb == 0, PSG_ERR_INVALID, "%s: null out", name);
  PSG_REQUIRE(nb > 0 || n == 0, PSG_ERR_INVALID, "%s: %llu keys and no bag to hold them", name,
              (unsigned long long)n);
  PSG_REQUIRE(mode == PSG_POOL_SUM || mode == PSG_POOL_MEAN, PSG_ERR_INVALID, "%s: mode %d is no pooling mode", name,
              mode);
  PSG_REQUIRE(mode != PSG_POOL_MEAN || !weights, PSG_ERR_INVALID, "%s: weights with PSG_POOL_MEAN", name);
  PSG_REQUIRE((reinterpret_cast<uintptr_t>(weights) & 3u) == 0, PSG_ERR_INVALID, "%s: weights not on a 4-B boundary",
              name);
  PSG_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, PSG_ERR_INVALID, "%s: out not on a 4-B boundary", name);
  PSG_TRY(q_require_count(name, n, "keys"));
  PSG_TRY(q_require_count(name, nb, "bags"));
  if (nb == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  PSG_TRY(q_gate_begin(q, n, st));
  PSG_TRY(rows_offsets_check(offsets, n, nb, q->gate, st));
  if (n) PSG_TRY(rows_resolve_any(keys, n, q->keys, q->size, q->key_begin, q->key_end, q->slots, q->gate, st));
  if (mode == PSG_POOL_MEAN) PSG_TRY(launch_qpool<kQMean>(q, offsets, nullptr, out, nullptr, nb, st));
  else if (weights) PSG_TRY(launch_qpool<kQWeighted>(q, offsets, weights, out, nullptr, nb, st));
  else PSG_TRY(launch_qpool<kQSum>(q, offsets, nullptr, out, nullptr, nb, st));
  // the one synchronisation: keys, offsets and weights no longer read, the reply in memory, the flags on the host
  return q_gate_end(q, name, n, st);
}

}  // extern "C"
