// row_ckpt_file.cpp — ps::SaveRowTable / ps::LoadRowTable (ps/row_checkpoint.h)
// on one GPU without a PS job: a table of `rows` F32 rows of `width` (Adam
// moments unless adam = 0) is written to `path`, read back whole into a second
// table and in two halves of the key range into a third and a fourth; all three
// ways must give back keys, rows and moments bit for bit (compared through
// psg_table_export and psg_checksum, inside HBM) and the iteration.  With
// enough rows the file takes several chunks of kRowCheckpointChunkBytes.
// Prints the wall time of the save and of the whole load: tools/rows_ckpt_bench.py
// reads that line.  Plain program: exits non-zero on a failed CHECK.
// With a fifth argument only the save and the whole load are run (a measurement).
// usage: row_ckpt_file width rows path [adam] [timing]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ps/row_checkpoint.h"

using namespace ps;

struct Table {
  psg_table* t = nullptr;
  Table(uint32_t w, bool adam) {
    device::Check(psg_table_create(PSG_F32, w, 0, kMaxKey, 0, &t), "psg_table_create");
    if (adam) device::Check(psg_table_set_adam(t, 0.01, 0.9, 0.999, 1e-8), "psg_table_set_adam");
  }
  ~Table() { psg_table_destroy(t); }
};

struct Buf {
  void* p = nullptr;
  explicit Buf(size_t bytes) { device::Check(psg_malloc(&p, bytes ? bytes : 8), "psg_malloc"); }
  ~Buf() { psg_free(p); }
};

// checksums of rows [first, first + count) of a table: keys, rows, m, v
struct Sums {
  uint64_t s[4] = {0, 0, 0, 0};
  bool operator==(const Sums& o) const { return s[0] == o.s[0] && s[1] == o.s[1] && s[2] == o.s[2] && s[3] == o.s[3]; }
};

static Sums SumsOf(psg_table* t, uint64_t first, uint64_t count, uint32_t w, bool adam) {
  Sums r;
  if (!count) return r;
  psg_stream st = device::ThreadStream();
  Buf k(count * 8), rows((count * w * 4 + 7) / 8 * 8), m(count * w * 8), v(count * w * 8);
  device::Check(psg_memset(rows.p, 0, (count * w * 4 + 7) / 8 * 8, st), "psg_memset");
  device::Check(psg_table_export(t, first, count, (uint64_t*)k.p, rows.p, adam ? (double*)m.p : nullptr,
                                 adam ? (double*)v.p : nullptr, st),
                "psg_table_export");
  device::Check(psg_checksum(k.p, count * 8, &r.s[0], st), "psg_checksum");
  device::Check(psg_checksum(rows.p, (count * w * 4 + 7) / 8 * 8, &r.s[1], st), "psg_checksum");
  if (adam) {
    device::Check(psg_checksum(m.p, count * w * 8, &r.s[2], st), "psg_checksum");
    device::Check(psg_checksum(v.p, count * w * 8, &r.s[3], st), "psg_checksum");
  }
  return r;
}

static uint64_t SizeOf(psg_table* t) {
  psg_table_info info;
  device::Check(psg_table_get_info(t, &info), "psg_table_get_info");
  return info.size;
}

int main(int argc, char** argv) {
  CHECK(argc >= 4) << "usage: row_ckpt_file width rows path [adam]";
  const uint32_t w = (uint32_t)std::atol(argv[1]);
  const uint64_t n = (uint64_t)std::atoll(argv[2]);
  const std::string path = argv[3];
  const bool adam = argc > 4 ? std::atol(argv[4]) != 0 : true;
  device::Check(psg_set_device(0), "psg_set_device");
  psg_stream st = device::ThreadStream();
  const Key step = kMaxKey / (n + 1);  // keys over the whole key range
  Table a(w, adam);
  {
    Buf k(n * 8), rows(n * w * 4), m(n * w * 8), v(n * w * 8);
    device::Check(psg_fill_keys_arith((uint64_t*)k.p, n, 1, step, st), "psg_fill_keys_arith");
    device::Check(psg_fill_synth(rows.p, n * w, PSG_F32, 1, 1, -1.0, 1.0, st), "psg_fill_synth");
    device::Check(psg_fill_synth(m.p, n * w, PSG_F64, 2, 1, -1.0, 1.0, st), "psg_fill_synth");
    device::Check(psg_fill_synth(v.p, n * w, PSG_F64, 3, 1, 0.0, 1e-3, st), "psg_fill_synth");
    device::Check(psg_table_assign(a.t, (const uint64_t*)k.p, rows.p, adam ? (const double*)m.p : nullptr,
                                   adam ? (const double*)v.p : nullptr, n, st),
                  "psg_table_assign");
  }
  CHECK_EQ(SizeOf(a.t), n);
  using Clock = std::chrono::steady_clock;
  auto ms = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
  auto t0 = Clock::now();
  SaveRowTable(a.t, 7, path);
  const double save_ms = ms(t0);
  Table b(w, adam);
  int it = -1;
  t0 = Clock::now();
  const int loaded = LoadRowTable(b.t, path, 0, kMaxKey, &it);
  const double load_ms = ms(t0);
  CHECK_EQ((uint64_t)loaded, n);
  CHECK_EQ(it, 7);
  CHECK_EQ(SizeOf(b.t), n);
  const Sums whole = SumsOf(a.t, 0, n, w, adam);
  CHECK(SumsOf(b.t, 0, n, w, adam) == whole) << "the loaded table differs from the saved one";
  const uint64_t file_bytes = 64 + n * (8 + (uint64_t)w * 4 + (adam ? (uint64_t)w * 16 : 0));
  auto report = [&]() {
    std::printf("row ckpt file ok: width %u rows %llu adam %d file_bytes %llu chunk_bytes %zu save_ms %.3f load_ms %.3f\n", w,
                (unsigned long long)n, adam ? 1 : 0, (unsigned long long)file_bytes, kRowCheckpointChunkBytes, save_ms,
                load_ms);
  };
  if (argc > 5) {
    report();
    return 0;
  }
  // two halves of the key range into two tables, as two servers load one file
  const uint64_t n_lo = n / 3;
  const Key mid = 1 + n_lo * step;  // the key of row n_lo
  Table lo(w, adam), hi(w, adam);
  CHECK_EQ((uint64_t)LoadRowTable(lo.t, path, 0, mid, nullptr), n_lo);
  CHECK_EQ((uint64_t)LoadRowTable(hi.t, path, mid, kMaxKey, nullptr), n - n_lo);
  CHECK(SumsOf(lo.t, 0, n_lo, w, adam) == SumsOf(a.t, 0, n_lo, w, adam)) << "the lower part differs";
  CHECK(SumsOf(hi.t, 0, n - n_lo, w, adam) == SumsOf(a.t, n_lo, n - n_lo, w, adam)) << "the upper part differs";
  // a table without Adam state takes the rows alone; an Adam table takes a file without moments
  Table other(w, !adam);
  CHECK_EQ((uint64_t)LoadRowTable(other.t, path, 0, kMaxKey, nullptr), n);
  const Sums rows_only = SumsOf(other.t, 0, n, w, false);
  CHECK(rows_only.s[0] == whole.s[0] && rows_only.s[1] == whole.s[1]) << "rows loaded without moments differ";
  report();
  return 0;
}
