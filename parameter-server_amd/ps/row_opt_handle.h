// ps/row_opt_handle.h — a server handle that trains rows of `width` floats per
// key in HBM: the async-mode LR server's handle on a row table.
//
// Reference: lr::LRServer::RequestHandle in async mode (tests/src/LRServer.h:
// 179-206) with Adam (tests/src/Adam.h:28-34), applied to the rows a gradient
// Push names instead of one dense weight vector:
//
//   Push, cmd 0 or 1:  width gradients per key, applied at once with the
//                      current iteration (psg_table_update: SGD, or Adam with
//                      its moments beside the rows); a PushPull answers with
//                      the updated rows.  After a Push with cmd == 1 from
//                      worker 0 is applied the iteration goes up by one
//                      (LRServer.h:193-195).
//   Push, cmd 2:       kAccumulate — row(key_i)[j] += vals[i * width + j]
//                      (psg_table_handle), how a worker seeds rows; the
//                      moments are untouched.
//   Pull:              res.vals[i * width + j] = row(key_i)[j].
//   Pull, cmd 3:       kRowLookup — the same without inserting: a key the table
//                      does not hold answers with a zero row (psg_table_lookup).
//   Push, cmd 4:       kRowErase — keys and no values: the named rows and their
//                      moments are removed at once (psg_table_erase); the
//                      iteration is untouched.  (Both: ps/row_handle.h.)
//   Pull, cmd 5:       kRowLookupPooled — keys in bags (KVWorker::ZPullPooled):
//                      one row per bag, the sum of its rows here; no insert.
//   Push, cmd 6 or 7:  kRowUpdatePooled / kRowUpdatePooledStep — keys in bags and
//                      one gradient row per bag (KVWorker::ZPushPooled), applied
//                      at once with the current iteration
//                      (psg_table_update_pooled); after a cmd 7 from worker 0
//                      the iteration goes up by one, as after its cmd 1.  With
//                      per-id weights (KVWorker::ZPushPooledWeighted):
//                      psg_table_update_pooled_weighted(weights, PSG_POOL_SUM),
//                      the step handled the same.  A mean Push
//                      (ZPushPooledMean) arrives divided: a plain cmd 6 / 7.
//   Pull, cmd 5 with weights, cmd 8:  the weighted and the mean lookup
//                      (ps/row_handle.h).
//
// The rows live in a psg_table over [0, kMaxKey), created on the first request
// (or by SaveModel / LoadModel, which write and read rows, moments and iteration);
// an absent key starts from a zero row and zero moments.  Adam gets
// ((double)learning_rate, 0.9, 0.999, 1e-8), as LRServer.h:83-84 constructs it.
// The iteration is the server's one counter, as in the reference: there is no
// per-row step count.  Keys must be strictly ascending (KVApp.h:23) unless the
// handle was built with any_order, when it calls psg_table_update_any /
// psg_table_handle_any and every occurrence of a key is applied in arrival
// order with the request's one iteration.  Register with
// KVServer::SetDeviceRequestHandle; host frames are staged into HBM.
#pragma once
#include <memory>
#include <string>

#include "ps/row_handle.h"

namespace ps {

struct KVServerRowOptHandle {
  static constexpr int kAccumulate = 2;  // cmd of a Push that adds to the rows instead of training them

  struct State {
    psg_table* table = nullptr;
    uint32_t width = 0;
    float lr = 0.01f;
    bool use_adam = false;
    int iteration = 0;
    bool any_order = false;
    detail::RowInit init;
    ~State() {
      if (table) psg_table_destroy(table);
    }
  };
  std::shared_ptr<State> state = std::make_shared<State>();

  KVServerRowOptHandle(uint32_t width, float learning_rate, bool use_adam, int start_iteration = 0,
                       bool any_order = false) {
    CHECK(width >= 1 && width <= 4096) << "KVServerRowOptHandle: width " << width << " outside [1, 4096]";
    CHECK_GE(start_iteration, 0);
    state->width = width;
    state->lr = learning_rate;
    state->use_adam = use_adam;
    state->iteration = start_iteration;
    state->any_order = any_order;
  }

  void operator()(const KVMeta& req_meta, const KVPairs<float>& req_data, KVServer<float>* server) {
    State& st = *state;
    const size_t n = req_data.keys.size();
    const size_t w = st.width;
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerRowOptHandle: the table lives in HBM and this node has no GPU";
    CHECK(req_data.lens.empty()) << "KVServerRowOptHandle: rows have one fixed width, lens are not supported";
    Table();
    // kRowLookup / kRowErase (ps/row_handle.h): no gradient, no iteration
    if (detail::ServeRowLifecycle("KVServerRowOptHandle", st.table, req_meta, req_data, server, w)) return;
    if (req_meta.push && (req_meta.cmd == kRowUpdatePooled || req_meta.cmd == kRowUpdatePooledStep)) {
      // one gradient row per bag, applied at once with the current iteration;
      // worker 0's kRowUpdatePooledStep ends an iteration, as its cmd 1 does
      const bool ends = req_meta.cmd == kRowUpdatePooledStep && req_meta.sender == PostOffice::WorkerRankToID(0);
      detail::ServeRowsPooled("KVServerRowOptHandle", req_meta, req_data, server, w, "server.handle.rows.update_pooled",
                              [&](psg_stream s, const Key* keys, const uint64_t* offsets, const float* weights,
                                  const float* grads, float*, size_t nb) {
                                if (weights)
                                  device::Check(psg_table_update_pooled_weighted(st.table, keys, offsets, weights,
                                                                                 PSG_POOL_SUM, grads, n, nb, st.lr,
                                                                                 st.iteration, s),
                                                "psg_table_update_pooled_weighted");
                                else
                                  device::Check(psg_table_update_pooled(st.table, keys, offsets, grads, n, nb, st.lr,
                                                                        st.iteration, s),
                                                "psg_table_update_pooled");
                              });
      if (ends) ++st.iteration;
      return;
    }
    const int flags = (req_meta.push ? PSG_PUSH : 0) | (req_meta.pull ? PSG_PULL : 0);
    const bool accumulate = req_meta.push && req_meta.cmd == kAccumulate;
    if (req_meta.push) {
      CHECK_EQ(n * w, req_data.vals.size()) << "a Push carries width values per key";
      CHECK(req_meta.cmd >= 0 && req_meta.cmd <= kAccumulate) << "KVServerRowOptHandle: unknown Push cmd " << req_meta.cmd;
    }
    // LRServer.h:193-195: worker 0's Push with cmd 1 ends an iteration, once it is applied
    const bool ends_iteration = req_meta.push && req_meta.cmd == 1 && req_meta.sender == PostOffice::WorkerRankToID(0);
    if (ends_iteration && n == 0) ++st.iteration;  // nothing to apply: ServeRows makes no call
    detail::ServeRows(
        req_meta, req_data, server, w,
        !req_meta.push ? "server.handle.rows.pull" : accumulate ? "server.handle.rows.push" : "server.handle.rows.update",
        [&](psg_stream s, const Key* keys, const float* vals, float* out) {
          if (req_meta.push && !accumulate)
            device::Check((st.any_order ? psg_table_update_any : psg_table_update)(st.table, flags, keys, vals, out, n,
                                                                                   st.lr, st.iteration, s),
                          st.any_order ? "psg_table_update_any" : "psg_table_update");
          else
            device::Check((st.any_order ? psg_table_handle_any : psg_table_handle)(st.table, flags, keys, vals, out, n, s),
                          st.any_order ? "psg_table_handle_any" : "psg_table_handle");
          if (ends_iteration) ++st.iteration;
        });
  }

  int iteration() const { return state->iteration; }
  // New rows start from seeded uniform values in [lo, hi] (detail::RowInit, ps/row_handle.h)
  void SetInit(uint64_t seed, float lo, float hi) { state->init.Set("KVServerRowOptHandle", state->table, seed, lo, hi); }
  // the rows the table holds now: a lookup leaves it as it is, an erase lowers it
  size_t size() const { return detail::RowTableSize(state->table); }

  // Rows, moments and the iteration to a file and back (ps/row_checkpoint.h; the
  // reference's SaveModel / USE_OLD_MODEL, LRServer.h:107-115, 36-63).  Called on
  // the server node between barriers, with no request in flight.  LoadModel
  // assigns the keys of this server's own range, SETS the iteration to the
  // file's and returns the rows loaded: call it once per saved shard, whatever
  // the number of servers that saved.
  void SaveModel(const std::string& path) { SaveRowTable(Table(), state->iteration, path); }
  int LoadModel(const std::string& path) { return detail::LoadOwnRows(Table(), path, &state->iteration); }

 private:
  psg_table* Table() {
    return detail::EnsureRowTable(&state->table, PSG_F32, state->width, state->use_adam, state->lr, &state->init);
  }
};

}  // namespace ps
