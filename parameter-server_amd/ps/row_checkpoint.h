// ps/row_checkpoint.h — a row table (psg_table) to a file and back: rows, Adam
// moments and the iteration count.
//
// Reference: lr::LRServer::SaveModel (tests/src/LRServer.h:107-115) writes the
// iteration count, the size and the weights as text; lr::InitWeight with
// USE_OLD_MODEL (LRServer.h:36-63) reads them back.  Here the model is a sparse
// table of rows, the file is binary so that every value comes back bit for bit,
// and the Adam moments are saved too: a resumed run is the uninterrupted one.
//
// File format, version 1: one file per table, little-endian, no padding.
//   offset  0  char     magic[8]     "PSGROWS1" (the digit is the format version)
//           8  uint32   dtype        PSG_F32 / F64 / F16 / BF16
//          12  uint32   width        elements per row
//          16  uint32   has_moments  1: m and v follow the rows
//          20  int32    iteration
//          24  float64  adam[4]      learning_rate, beta1, beta2, epsilon of the
//                                    saved table (zeros without Adam state);
//                                    for the reader's information, never loaded
//          56  uint64   n            rows
//          64  uint64   keys[n]      strictly ascending
//              dtype    rows[n * width]
//              float64  m[n * width], v[n * width]    if has_moments; plain
//                                    column order, as psg_table_dump_moments
//
// Both directions move the table in chunks of at most kRowCheckpointChunkBytes
// through one device buffer and one pinned host buffer of that size
// (psg_table_export / psg_table_assign): host memory does not grow with the
// table, except for the file's key array while it is loaded (8 B a row).  A
// load of more than one chunk first inserts its keys with one psg_table_assign
// without rows (the keys in HBM for that call), so the table is merged once.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>
#include <vector>

#include "internal/device.h"
#include "ps/base.h"
#include "ps/log.h"

namespace ps {

constexpr size_t kRowCheckpointChunkBytes = 16u << 20;  // of keys, rows and moments together (at least one row)

namespace detail {

struct RowFileHeader {
  char magic[8];
  uint32_t dtype, width, has_moments;
  int32_t iteration;
  double adam[4];
  uint64_t n;
};
static_assert(sizeof(RowFileHeader) == 64, "the header is 64 bytes without padding");
constexpr char kRowFileMagic[9] = "PSGROWS1";

inline size_t RowElemSize(int dtype) { return dtype == PSG_F64 ? 8 : dtype == PSG_F32 ? 4 : 2; }

struct Fd {  // closed on every path: a failed CHECK throws
  int fd = -1;
  ~Fd() {
    if (fd >= 0) ::close(fd);
  }
};

inline void WriteAt(int fd, const void* p, size_t bytes, uint64_t off, const std::string& path) {
  const char* c = (const char*)p;
  while (bytes) {
    const ssize_t w = ::pwrite(fd, c, bytes, (off_t)off);
    CHECK(w > 0) << "writing " << path << ": " << std::strerror(errno);
    c += w, off += (uint64_t)w, bytes -= (size_t)w;
  }
}

inline void ReadAt(int fd, void* p, size_t bytes, uint64_t off, const std::string& path) {
  char* c = (char*)p;
  while (bytes) {
    const ssize_t r = ::pread(fd, c, bytes, (off_t)off);
    CHECK(r > 0) << "reading " << path << (r == 0 ? ": the file ends early" : std::strerror(errno));
    c += r, off += (uint64_t)r, bytes -= (size_t)r;
  }
}

// One chunk of c rows in a buffer: keys, rows, m, v, each on 16 B.  The same
// offsets hold in the device buffer and in the pinned host buffer, so a chunk
// crosses PCIe in one copy.
struct RowChunk {
  size_t row_bytes, mom_bytes;  // per row; mom_bytes: one of m / v, 0 without moments
  size_t rows;                  // rows a chunk holds
  size_t keys_off = 0, rows_off, m_off, v_off, bytes;
  // `want`: the rows to move in all; a smaller table gets smaller buffers
  RowChunk(size_t width, size_t esize, bool moments, uint64_t want) {
    row_bytes = width * esize;
    mom_bytes = moments ? width * sizeof(double) : 0;
    rows = std::max<size_t>(1, (kRowCheckpointChunkBytes - 64) / (sizeof(Key) + row_bytes + 2 * mom_bytes));
    rows = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(rows, want));
    auto up = [](size_t x) { return (x + 15) & ~size_t(15); };
    rows_off = up(rows * sizeof(Key));
    m_off = up(rows_off + rows * row_bytes);
    v_off = up(m_off + rows * mom_bytes);
    bytes = up(v_off + rows * mom_bytes);
  }
};

struct RowStaging {  // the two buffers, freed on every path
  char* dev = nullptr;
  char* host = nullptr;
  explicit RowStaging(size_t bytes, bool with_host = true) {
    device::Check(psg_malloc((void**)&dev, bytes), "psg_malloc");
    if (with_host) device::Check(psg_host_alloc((void**)&host, bytes), "psg_host_alloc");
  }
  ~RowStaging() {
    if (dev) (void)psg_free(dev);
    if (host) (void)psg_host_free(host);
  }
};

}  // namespace detail

/* Write the whole table to `path` (replaced if it exists).  `iteration` is the
 * caller's count: a table does not know it. */
inline void SaveRowTable(psg_table* table, int iteration, const std::string& path) {
  using namespace detail;
  CHECK_NOTNULL(table);
  psg_table_info info;
  device::Check(psg_table_get_info(table, &info), "psg_table_get_info");
  RowFileHeader h = {};
  std::memcpy(h.magic, kRowFileMagic, 8);
  int has_adam = 0;
  device::Check(psg_table_get_adam(table, &has_adam, h.adam), "psg_table_get_adam");
  h.dtype = (uint32_t)info.dtype;
  h.width = info.width;
  h.has_moments = has_adam ? 1 : 0;
  h.iteration = iteration;
  h.n = info.size;
  Fd f;
  f.fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  CHECK(f.fd >= 0) << "SaveRowTable: cannot create " << path << ": " << std::strerror(errno);
  WriteAt(f.fd, &h, sizeof(h), 0, path);
  const RowChunk c(info.width, RowElemSize(info.dtype), has_adam != 0, h.n);
  const uint64_t keys_at = sizeof(h), rows_at = keys_at + h.n * sizeof(Key);
  const uint64_t m_at = rows_at + h.n * c.row_bytes, v_at = m_at + h.n * c.mom_bytes;
  if (h.n == 0) return;
  RowStaging s(c.bytes);
  psg_stream st = device::ThreadStream();
  for (uint64_t first = 0; first < h.n; first += c.rows) {
    const uint64_t cnt = std::min<uint64_t>(c.rows, h.n - first);
    device::Check(psg_table_export(table, first, cnt, (uint64_t*)(s.dev + c.keys_off), s.dev + c.rows_off,
                                   has_adam ? (double*)(s.dev + c.m_off) : nullptr,
                                   has_adam ? (double*)(s.dev + c.v_off) : nullptr, st),
                  "psg_table_export");
    device::Check(psg_memcpy(s.host, s.dev, c.bytes, 1, st), "psg_memcpy");
    device::Check(psg_stream_sync(st), "psg_stream_sync");
    WriteAt(f.fd, s.host + c.keys_off, cnt * sizeof(Key), keys_at + first * sizeof(Key), path);
    WriteAt(f.fd, s.host + c.rows_off, cnt * c.row_bytes, rows_at + first * c.row_bytes, path);
    if (has_adam) {
      WriteAt(f.fd, s.host + c.m_off, cnt * c.mom_bytes, m_at + first * c.mom_bytes, path);
      WriteAt(f.fd, s.host + c.v_off, cnt * c.mom_bytes, v_at + first * c.mom_bytes, path);
    }
  }
  CHECK(::fsync(f.fd) == 0) << "SaveRowTable: " << path << ": " << std::strerror(errno);
}

/* Assign the file's rows whose keys are in [key_begin, key_end) to the table
 * (psg_table_assign: rows as bytes, absent keys inserted).  The moments are
 * loaded when the file has them and the table has Adam state; otherwise the
 * rows alone, and an Adam table's inserted rows start from zero moments (what
 * USE_OLD_MODEL leaves of the reference's Adam).  A dtype or width that
 * differs from the table's fails a CHECK before anything is written.
 * *iteration (may be null) gets the file's count.  Returns the rows loaded. */
inline int LoadRowTable(psg_table* table, const std::string& path, Key key_begin, Key key_end, int* iteration) {
  using namespace detail;
  CHECK_NOTNULL(table);
  psg_table_info info;
  device::Check(psg_table_get_info(table, &info), "psg_table_get_info");
  int has_adam = 0;
  device::Check(psg_table_get_adam(table, &has_adam, nullptr), "psg_table_get_adam");
  Fd f;
  f.fd = ::open(path.c_str(), O_RDONLY);
  CHECK(f.fd >= 0) << "LoadRowTable: cannot open " << path << ": " << std::strerror(errno);
  RowFileHeader h;
  ReadAt(f.fd, &h, sizeof(h), 0, path);
  CHECK(std::memcmp(h.magic, kRowFileMagic, 8) == 0) << "LoadRowTable: " << path << " is not a row table file of version 1";
  CHECK_EQ((int)h.dtype, info.dtype) << "LoadRowTable: dtype of " << path << " and of the table";
  CHECK_EQ(h.width, info.width) << "LoadRowTable: width of " << path << " and of the table";
  CHECK(h.has_moments <= 1 && h.iteration >= 0) << "LoadRowTable: bad header in " << path;
  const bool file_moments = h.has_moments != 0;
  const bool moments = file_moments && has_adam;
  const size_t row_bytes = info.width * RowElemSize(info.dtype);
  const size_t file_mom_bytes = file_moments ? info.width * sizeof(double) : 0;
  const uint64_t keys_at = sizeof(h), rows_at = keys_at + h.n * sizeof(Key);
  const uint64_t m_at = rows_at + h.n * row_bytes, v_at = m_at + h.n * file_mom_bytes;
  const off_t end = ::lseek(f.fd, 0, SEEK_END);
  CHECK_EQ((uint64_t)end, v_at + h.n * file_mom_bytes) << "LoadRowTable: size of " << path;
  if (iteration) *iteration = h.iteration;
  std::vector<Key> keys(h.n);
  if (h.n) ReadAt(f.fd, keys.data(), h.n * sizeof(Key), keys_at, path);
  // the keys are sorted: this range's stretch of them
  const uint64_t lo = std::lower_bound(keys.begin(), keys.end(), key_begin) - keys.begin();
  const uint64_t hi = std::lower_bound(keys.begin() + lo, keys.end(), key_end) - keys.begin();
  if (lo == hi) return 0;
  const RowChunk c(info.width, RowElemSize(info.dtype), moments, hi - lo);
  RowStaging s(c.bytes);
  psg_stream st = device::ThreadStream();
  if (hi - lo > c.rows) {
    // more than one chunk: the stretch's keys go in first, all at once (8 B a
    // row of HBM for the moment), so the table is merged once and not per chunk
    RowStaging all((hi - lo) * sizeof(Key), false);
    for (uint64_t first = lo; first < hi; first += c.rows) {
      const uint64_t cnt = std::min<uint64_t>(c.rows, hi - first);
      std::memcpy(s.host, keys.data() + first, cnt * sizeof(Key));
      device::Check(psg_memcpy(all.dev + (first - lo) * sizeof(Key), s.host, cnt * sizeof(Key), 0, st), "psg_memcpy");
      device::Check(psg_stream_sync(st), "psg_stream_sync");
    }
    device::Check(psg_table_assign(table, (const uint64_t*)all.dev, nullptr, nullptr, nullptr, hi - lo, st),
                  "psg_table_assign");
  }
  for (uint64_t first = lo; first < hi; first += c.rows) {
    const uint64_t cnt = std::min<uint64_t>(c.rows, hi - first);
    std::memcpy(s.host + c.keys_off, keys.data() + first, cnt * sizeof(Key));
    ReadAt(f.fd, s.host + c.rows_off, cnt * c.row_bytes, rows_at + first * c.row_bytes, path);
    if (moments) {
      ReadAt(f.fd, s.host + c.m_off, cnt * c.mom_bytes, m_at + first * c.mom_bytes, path);
      ReadAt(f.fd, s.host + c.v_off, cnt * c.mom_bytes, v_at + first * c.mom_bytes, path);
    }
    device::Check(psg_memcpy(s.dev, s.host, c.bytes, 0, st), "psg_memcpy");
    // returns when the chunk is no longer read: the buffers are free for the next
    device::Check(psg_table_assign(table, (const uint64_t*)(s.dev + c.keys_off), s.dev + c.rows_off,
                                   moments ? (const double*)(s.dev + c.m_off) : nullptr,
                                   moments ? (const double*)(s.dev + c.v_off) : nullptr, cnt, st),
                  "psg_table_assign");
  }
  return (int)(hi - lo);
}

}  // namespace ps
