// ps/row_handle.h — a server handle that keeps a row of `width` values per key
// in HBM (embedding rows).
//
// Reference: KVServerDefaultHandle's loop (src/ps/KVApp.h:446-454) for the
// requests a worker sends with k = vals.size() / keys.size() values per key,
// which DefaultSlicer already slices per server (src/ps/KVApp.h:515-574) and
// the pull merge concatenates; the reference's default handle CHECKs
// n == vals.size() (KVApp.h:441) and so cannot keep them.
//
//   Push:  row(key_i)[j] += vals[i * width + j]
//   Pull:  res.vals[i * width + j] = row(key_i)[j]    (post-update)
//   Pull, cmd kRowLookup:  the same without inserting the keys it has not seen
//   Push, cmd kRowErase:   keys and no values: the named rows are removed
//   Pull, cmd kRowLookupPooled:  keys in bags: one row per bag, its rows summed
//
// The rows live in a psg_table over [0, kMaxKey), created on the first
// request (or by SaveModel / LoadModel, below); an absent key is inserted with
// a zero row or, after SetInit, with its seeded initial row
// (psg_table_set_init).  By default keys must be
// strictly ascending (the KVPairs contract, KVApp.h:23): a list out of order or
// with repeats fails the request's CHECK.  With any_order set the handle calls
// psg_table_handle_any, which serves such a list in arrival order, every
// occurrence of a key on its own, as the scalar default handle does.  Register with KVServer::SetDeviceRequestHandle, so
// HBM frames are read in place; host frames are staged into HBM.  The handle
// has no run handle: every request is served on its own, and workers slice
// their key lists for real.
#pragma once
#include <memory>
#include <string>

#include "ps/kv_app.h"
#include "ps/row_checkpoint.h"

namespace ps {

// Request cmds the three row handles share, next to their kAccumulate (2):
//   kRowLookup, on a Pull:  answered through psg_table_lookup — the rows of the
//                           keys the table holds, zero rows for the others, in
//                           any order and with repeats, and NOTHING is inserted
//                           (a plain Pull inserts every key it has not seen);
//   kRowErase, on a Push:   keys and no values; the keys the table holds are
//                           removed at once (psg_table_erase), in any order.
//                           It never counts towards a round or an iteration.
// A PushPull with either fails the handle's CHECK.
constexpr int kRowLookup = 3;
constexpr int kRowErase = 4;
// The pooled cmds (ps/kv_app.h: kRowLookupPooled = 5, kRowUpdatePooled = 6,
// kRowUpdatePooledStep = 7), sent by KVWorker::ZPullPooled / ZPushPooled with the
// request's bag offsets (KVPairs::offsets):
//   kRowLookupPooled, on a Pull:  psg_table_lookup_pooled on this server's share
//                           of every bag: nb * width values, one row per bag,
//                           nothing inserted; all three handles serve it;
//   kRowUpdatePooled, kRowUpdatePooledStep, on a Push:  keys, offsets and one
//                           gradient row per bag; KVServerRowOptHandle applies
//                           them at once (psg_table_update_pooled),
//                           KVServerRowSyncHandle holds them for its round
//                           (psg_table_update_pooled_merged), KVServerRowHandle
//                           fails a CHECK that says so.
// With per-id weights (KVPairs::weights, KVWorker::ZPullPooledWeighted /
// ZPushPooledWeighted) cmd 5 is psg_table_lookup_pooled_weighted(weights,
// PSG_POOL_SUM) and cmd 6 / 7 psg_table_update_pooled_weighted on the optimizer
// handle; the sync handle refuses a weighted Push (a round's frames carry none).
//   kRowLookupPooledMean (8), on a Pull:  KVWorker::ZPullPooledMean to ONE server:
//                           psg_table_lookup_pooled_weighted(NULL, PSG_POOL_MEAN),
//                           the whole bags' mean; weights with it fail a CHECK.
//                           (Over several servers a mean is cmd 5 and the
//                           worker's division; a mean Push is a plain cmd 6 / 7.)
// A PushPull with any of these fails the handle's CHECK.

namespace detail {

// What the three row handles' SetInit(seed, lo, hi) keeps until the table is
// created: every new row starts from a uniform value in [lo, hi] that depends
// on (seed, key, column) alone (psg_table_set_init) instead of from zero, and
// kRowLookup and the pooled lookups answer a key the table does not hold with
// that row.  Called before the first request, with the same triple on every
// server: a row then does not depend on the number of servers.  The checkpoint
// file does not carry the triple (like the Adam parameters, it is the
// caller's to set again): a job resumed with the same triple is the
// uninterrupted job bit for bit, with another one the keys it has not seen yet
// start elsewhere.
struct RowInit {
  bool set = false;
  uint64_t seed = 0;
  float lo = 0.f, hi = 0.f;
  void Set(const char* who, psg_table* table, uint64_t seed_, float lo_, float hi_) {
    CHECK(!table) << who << "::SetInit comes before the first request, SaveModel or LoadModel: the table exists";
    CHECK(!set) << who << "::SetInit was called twice";
    set = true, seed = seed_, lo = lo_, hi = hi_;
  }
};

// The row handles' table, created on first use (a request, SaveModel or
// LoadModel): [0, kMaxKey), no rows allocated; with_adam gives it the moments
// of Adam(learning_rate), as LRServer.h:83-84 constructs it; init, where set,
// its initializer.
inline psg_table* EnsureRowTable(psg_table** table, int dtype, uint32_t width, bool with_adam = false,
                                 float learning_rate = 0.f, const RowInit* init = nullptr) {
  if (*table) return *table;
  device::Check(psg_table_create(dtype, width, 0, kMaxKey, 0, table), "psg_table_create");
  if (with_adam) device::Check(psg_table_set_adam(*table, (double)learning_rate, 0.9, 0.999, 1e-8), "psg_table_set_adam");
  if (init && init->set)
    device::Check(psg_table_set_init(*table, PSG_INIT_UNIFORM, init->seed, init->lo, init->hi), "psg_table_set_init");
  return *table;
}

// LoadModel's body: the file's rows in this server's own key range
// (PostOffice::GetServerRanges) into the table; the file's iteration count.
inline int LoadOwnRows(psg_table* table, const std::string& path, int* iteration) {
  PostOffice* po = PostOffice::Get();
  CHECK(po->is_server()) << "LoadModel is called on a server node";
  const Range& own = po->GetServerRanges()[po->my_rank()];
  return LoadRowTable(table, path, own.begin, own.end, iteration);
}

// The body the row handles share.  Stages the request's keys and values into
// HBM, takes the worker's own output slice or allocates the reply, runs
// call(stream, keys, vals, out) under a stage::Scope and answers.  call wraps a
// psg_table_* request, which returns once keys and vals are no longer read and
// the reply is in memory.
template <typename Value, typename Call>
void ServeRows(const KVMeta& req_meta, const KVPairs<Value>& req_data, KVServer<Value>* server, size_t width,
               const char* scope, Call call) {
  const size_t n = req_data.keys.size();
  const int dev = PostOffice::Get()->device();
  KVPairs<Value> res;
  SVector<Value> dout;
  bool direct = false;
  if (n && (req_meta.push || req_meta.pull)) {
    psg_stream s = device::ThreadStream();
    SVector<Key> dkeys = ToDeviceAsync(req_data.keys, dev);
    SVector<Value> dvals;
    if (req_meta.push) dvals = ToDeviceAsync(req_data.vals, dev);
    if (req_meta.pull) {
      // the worker's own output slice when it offered one of n * width
      // values (written in place: no reply frame, no merge)
      dout = server->TakeDirectOut(n * width);
      direct = !dout.empty();
      if (!direct) dout = SVector<Value>::OnDevice(n * width, dev);
    }
    stage::Scope t(scope);
    call(s, dkeys.data(), dvals.data(), dout.data());
  }
  if (req_meta.pull) {
    res.keys = req_data.keys;
    if (!direct) res.vals = req_data.keys.on_device() ? dout : ToHost(dout);
  }
  server->Response(req_meta, res);
}

// ServeRows for a pooled request (KVPairs::offsets: nb + 1 bag offsets into the
// keys): a Pull answers nb * width values, into the frame the worker offered
// when there is one; a Push carries nb * width values.  call(stream, keys,
// offsets, weights, vals, out, nb) wraps psg_table_lookup_pooled / _update_pooled
// or their weighted forms; weights: the request's, in HBM, or null without.
template <typename Value, typename Call>
void ServeRowsPooled(const char* who, const KVMeta& req_meta, const KVPairs<Value>& req_data, KVServer<Value>* server,
                     size_t width, const char* scope, Call call) {
  CHECK(!req_data.offsets.empty()) << who << ": cmd " << req_meta.cmd << " needs the bag offsets of a pooled request "
                                   << "(KVWorker::ZPullPooled / ZPushPooled)";
  const size_t nb = req_data.offsets.size() - 1;
  const int dev = PostOffice::Get()->device();
  if (req_meta.push)
    CHECK_EQ(nb * width, req_data.vals.size()) << who << ": a pooled Push carries width values per bag";
  if (!req_data.weights.empty())
    CHECK_EQ(req_data.weights.size(), req_data.keys.size()) << who << ": a weighted pooled request carries one weight per key";
  KVPairs<Value> res;
  SVector<Value> dout;
  bool direct = false;
  if (nb) {
    psg_stream s = device::ThreadStream();
    SVector<Key> dkeys = ToDeviceAsync(req_data.keys, dev);
    SVector<uint64_t> doffs = ToDeviceAsync(req_data.offsets, dev);
    SVector<float> dweights = ToDeviceAsync(req_data.weights, dev);
    SVector<Value> dvals;
    if (req_meta.push) dvals = ToDeviceAsync(req_data.vals, dev);
    if (req_meta.pull) {
      dout = server->TakeDirectOut(nb * width);
      direct = !dout.empty();
      if (!direct) dout = SVector<Value>::OnDevice(nb * width, dev);
    }
    stage::Scope t(scope);
    call(s, dkeys.data(), doffs.data(), dweights.empty() ? nullptr : dweights.data(), dvals.data(), dout.data(), nb);
  }
  if (req_meta.pull) {
    res.keys = req_data.keys;
    if (!direct) res.vals = req_data.keys.on_device() ? dout : ToHost(dout);
  }
  server->Response(req_meta, res);
}

// The accumulate handle trains no row on a pooled gradient, weighted or not:
// called first, on the host, before the request touches the device.
inline void RefusePooledUpdate(const char* who, const KVMeta& req_meta) {
  CHECK(!(req_meta.push && (req_meta.cmd == kRowUpdatePooled || req_meta.cmd == kRowUpdatePooledStep)))
      << who << ": a pooled update (cmd " << req_meta.cmd << ", KVWorker::ZPushPooled) is served by KVServerRowOptHandle "
      << "only; this handle does not merge pooled frames";
}

// A request with kRowLookup, kRowErase, kRowLookupPooled or kRowLookupPooledMean,
// served; false: it is none of them (the pooled updates are the optimizer
// handle's own).
template <typename Value>
bool ServeRowLifecycle(const char* who, psg_table* table, const KVMeta& req_meta, const KVPairs<Value>& req_data,
                       KVServer<Value>* server, size_t width) {
  const int cmd = req_meta.cmd;
  if (cmd != kRowLookup && cmd != kRowErase && !(cmd >= kRowLookupPooled && cmd <= kRowLookupPooledMean)) return false;
  CHECK(!(req_meta.push && req_meta.pull))
      << who << ": a PushPull cannot carry cmd " << cmd
      << " (kRowLookup and the pooled lookups go with a Pull, kRowErase and the pooled updates with a Push)";
  const size_t n = req_data.keys.size();
  if (req_meta.pull && cmd == kRowLookupPooled && req_data.weights.empty()) {
    ServeRowsPooled(who, req_meta, req_data, server, width, "server.handle.rows.lookup_pooled",
                    [&](psg_stream s, const Key* keys, const uint64_t* offsets, const float*, const Value*, Value* out,
                        size_t nb) {
                      device::Check(psg_table_lookup_pooled(table, keys, offsets, out, n, nb, s),
                                    "psg_table_lookup_pooled");
                    });
    return true;
  }
  if (req_meta.pull && (cmd == kRowLookupPooled || cmd == kRowLookupPooledMean)) {
    const bool mean = cmd == kRowLookupPooledMean;
    CHECK(!(mean && !req_data.weights.empty())) << who << ": a mean lookup (cmd " << cmd << ") takes no weights";
    ServeRowsPooled(who, req_meta, req_data, server, width, "server.handle.rows.lookup_pooled",
                    [&](psg_stream s, const Key* keys, const uint64_t* offsets, const float* weights, const Value*,
                        Value* out, size_t nb) {
                      device::Check(psg_table_lookup_pooled_weighted(table, keys, offsets, weights,
                                                                     mean ? PSG_POOL_MEAN : PSG_POOL_SUM, out, n, nb, s),
                                    "psg_table_lookup_pooled_weighted");
                    });
    return true;
  }
  if (req_meta.pull && cmd == kRowLookup) {
    ServeRows(req_meta, req_data, server, width, "server.handle.rows.lookup",
              [&](psg_stream s, const Key* keys, const Value*, Value* out) {
                device::Check(psg_table_lookup(table, keys, out, nullptr, n, s), "psg_table_lookup");
              });
    return true;
  }
  if (req_meta.push && cmd == kRowErase) {
    CHECK(req_data.vals.empty()) << who << ": a Push with kRowErase carries keys and no values, this one "
                                 << req_data.vals.size();
    ServeRows(req_meta, req_data, server, width, "server.handle.rows.erase",
              [&](psg_stream s, const Key* keys, const Value*, Value*) {
                device::Check(psg_table_erase(table, keys, n, nullptr, s), "psg_table_erase");
              });
    return true;
  }
  return false;  // a Pull with kRowErase, a Push with kRowLookup: the cmd means nothing there
}

// The rows a handle's table holds now (0 before its first request).
inline size_t RowTableSize(psg_table* table) {
  if (!table) return 0;
  psg_table_info info;
  device::Check(psg_table_get_info(table, &info), "psg_table_get_info");
  return (size_t)info.size;
}

}  // namespace detail

template <typename Value>
struct KVServerRowHandle {
  struct State {
    psg_table* table = nullptr;
    uint32_t width = 0;
    bool any_order = false;
    detail::RowInit init;
    ~State() {
      if (table) psg_table_destroy(table);
    }
  };
  std::shared_ptr<State> state = std::make_shared<State>();

  explicit KVServerRowHandle(uint32_t width, bool any_order = false) {
    CHECK(width >= 1 && width <= 4096) << "KVServerRowHandle: width " << width << " outside [1, 4096]";
    state->width = width;
    state->any_order = any_order;
  }

  void operator()(const KVMeta& req_meta, const KVPairs<Value>& req_data, KVServer<Value>* server) {
    const size_t n = req_data.keys.size();
    const size_t w = state->width;
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerRowHandle: the table lives in HBM and this node has no GPU";
    constexpr int dt = device::DType<Value>();
    CHECK_GE(dt, 0) << "KVServerRowHandle: value type not supported by the HBM table";
    CHECK(req_data.lens.empty()) << "KVServerRowHandle: rows have one fixed width, lens are not supported";
    detail::RefusePooledUpdate("KVServerRowHandle", req_meta);
    Table();
    if (detail::ServeRowLifecycle("KVServerRowHandle", state->table, req_meta, req_data, server, w)) return;
    const int flags = (req_meta.push ? PSG_PUSH : 0) | (req_meta.pull ? PSG_PULL : 0);
    if (req_meta.push) CHECK_EQ(n * w, req_data.vals.size()) << "a Push carries width values per key";
    detail::ServeRows(req_meta, req_data, server, w,
                      req_meta.push ? "server.handle.rows.push" : "server.handle.rows.pull",
                      [&](psg_stream s, const Key* keys, const Value* vals, Value* out) {
                        if (state->any_order)
                          device::Check(psg_table_handle_any(state->table, flags, keys, vals, out, n, s),
                                        "psg_table_handle_any");
                        else
                          device::Check(psg_table_handle(state->table, flags, keys, vals, out, n, s),
                                        "psg_table_handle");
                      });
  }

  // the rows the table holds now: a lookup leaves it as it is, an erase lowers it
  size_t size() const { return detail::RowTableSize(state->table); }

  // New rows start from seeded uniform values in [lo, hi] (detail::RowInit above)
  void SetInit(uint64_t seed, float lo, float hi) { state->init.Set("KVServerRowHandle", state->table, seed, lo, hi); }

  // The table to a file and back (ps/row_checkpoint.h; the reference's
  // SaveModel / USE_OLD_MODEL, LRServer.h:107-115, 36-63).  Called on the server
  // node between barriers, with no request in flight.  LoadModel assigns the
  // keys of this server's own range and returns their number: call it once per
  // saved shard, whatever the number of servers that saved.  An accumulate
  // handle has no iteration: it saves 0.
  void SaveModel(const std::string& path) { SaveRowTable(Table(), 0, path); }
  int LoadModel(const std::string& path) { return detail::LoadOwnRows(Table(), path, nullptr); }

 private:
  psg_table* Table() {
    return detail::EnsureRowTable(&state->table, device::DType<Value>(), state->width, false, 0.f, &state->init);
  }
};

}  // namespace ps
