// ps/row_sync_handle.h — a server handle that trains rows of `width` floats per
// key in HBM in rounds: the sync-mode LR server's handle on a row table, next to
// KVServerRowOptHandle (ps/row_opt_handle.h), which is its async mode.
//
// Reference: lr::LRServer::RequestHandle in sync mode (tests/src/LRServer.h:
// 151-178) with Adam (tests/src/Adam.h:28-34): every worker's gradient Push is
// merged into a buffer that starts from zero, in arrival order, and answered
// only when NumWorkers() Pushes have arrived; then the optimizer runs once on
// the sum and every held request is answered.  Here the gradients are rows:
//
//   Push, cmd 0 or 1:  width gradients per key.  The request is staged into HBM
//                      and held — its meta, keys, values and, for a PushPull,
//                      the worker's own output slice, taken at that moment.
//                      When PostOffice::num_workers() Pushes are held, ONE
//                      psg_table_update_merged call serves the round: per key
//                      the held gradients are summed from zero in arrival
//                      order, then one SGD / Adam step.  Then every held
//                      request is answered; a PushPull is answered ONCE, with
//                      the updated rows of its keys (the reference answers its
//                      pull half at once with the weights of before the round,
//                      and then answers again).
//   Push, cmd 2:       kAccumulate — row(key_i)[j] += vals[i * width + j], at
//                      once (psg_table_handle_any); the moments are untouched.
//   Pull:              res.vals[i * width + j] = row(key_i)[j], at once.
//   Pull, cmd 3:       kRowLookup — the same without inserting: a key the table
//                      does not hold answers with a zero row (psg_table_lookup).
//   Push, cmd 4:       kRowErase — keys and no values: the named rows and their
//                      moments are removed at once (psg_table_erase); it is not
//                      held, does not count towards the round and leaves the
//                      iteration alone.  (Both: ps/row_handle.h.)
//   Pull, cmd 5:       kRowLookupPooled — keys in bags (KVWorker::ZPullPooled):
//                      one row per bag, at once; nothing is inserted.
//   Push, cmd 6 or 7:  kRowUpdatePooled / kRowUpdatePooledStep — keys in bags and
//                      one gradient row per bag (KVWorker::ZPushPooledAll).  Staged
//                      with its offsets and held; it counts towards the round as
//                      a cmd 0 / 1 Push does, also with no key of this server's
//                      in it.  A round that holds one is served by ONE
//                      psg_table_update_pooled_merged call over pooled and plain
//                      frames alike (the bag's gradient row stands for every id
//                      of the bag; no expanded frame is ever built); then every
//                      held plain PushPull is answered with a Pull of its keys
//                      (psg_table_handle_any): the updated row for every
//                      occurrence, the bytes psg_table_update_merged's Pull leg
//                      gives.  A round without one is exactly the call above.
//                      A mean Push (KVWorker::ZPushPooledMeanAll) arrives divided
//                      and is such a frame.  A WEIGHTED pooled Push fails a CHECK
//                      before it is held: a round's frames carry no weights
//                      (psg_table_update_pooled_merged has none).
//   Pull, cmd 5 with weights, cmd 8:  the weighted and the mean lookup, at once
//                      (ps/row_handle.h).
//
// The iteration goes up by one after a round is applied, if the round held
// worker 0's Push with cmd == 1 or kRowUpdatePooledStep.  The reference counts when that Push arrives
// (LRServer.h:193-195), so whether the round it closes or the next one sees the
// new count depends on arrival order; counting after the round is the order
// "worker 0 arrives last", and a round's result does not depend on arrival.
//
// Key lists may come in any order and repeat, inside a request and across the
// round's requests.  A round merges at most 16 requests: more workers fail the
// handle's CHECK.  The rows live in a psg_table over [0, kMaxKey), created on
// the first request (or by SaveModel / LoadModel); an absent key starts from a
// zero row (after SetInit: its seeded initial row, psg_table_set_init) and zero moments.
// Adam gets ((double)learning_rate, 0.9, 0.999, 1e-8), as LRServer.h:83-84
// constructs it.  Register with KVServer::SetDeviceRequestHandle; host frames
// are staged into HBM.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "ps/row_handle.h"

namespace ps {

struct KVServerRowSyncHandle {
  static constexpr int kAccumulate = 2;  // cmd of a Push that adds to the rows instead of training them
  static constexpr int kMaxWorkers = 16;  // frames one psg_table_update_merged call merges

  struct Held {  // one gradient Push of the round under way
    KVMeta meta;
    SVector<Key> keys;     // as received (the reply's keys; alive until its staging copy has run)
    SVector<float> vals;
    SVector<Key> dkeys;    // in HBM
    SVector<float> dvals;
    SVector<float> dout;   // a PushPull's reply: the worker's own slice (direct) or ours
    bool direct = false;
    bool pooled = false;         // cmd kRowUpdatePooled / kRowUpdatePooledStep: vals hold one row per bag
    SVector<uint64_t> offsets;   // its nb + 1 bag offsets, as received
    SVector<uint64_t> doffsets;  // in HBM
    size_t nb = 0;
  };
  struct State {
    psg_table* table = nullptr;
    uint32_t width = 0;
    float lr = 0.01f;
    bool use_adam = false;
    int iteration = 0;
    std::vector<Held> held;
    detail::RowInit init;
    ~State() {
      if (table) psg_table_destroy(table);
    }
  };
  std::shared_ptr<State> state = std::make_shared<State>();

  KVServerRowSyncHandle(uint32_t width, float learning_rate, bool use_adam, int start_iteration = 0) {
    CHECK(width >= 1 && width <= 4096) << "KVServerRowSyncHandle: width " << width << " outside [1, 4096]";
    CHECK_GE(start_iteration, 0);
    state->width = width;
    state->lr = learning_rate;
    state->use_adam = use_adam;
    state->iteration = start_iteration;
  }

  void operator()(const KVMeta& req_meta, const KVPairs<float>& req_data, KVServer<float>* server) {
    State& st = *state;
    const size_t n = req_data.keys.size();
    const size_t w = st.width;
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerRowSyncHandle: the table lives in HBM and this node has no GPU";
    CHECK(req_data.lens.empty()) << "KVServerRowSyncHandle: rows have one fixed width, lens are not supported";
    const int nw = PostOffice::Get()->num_workers();
    CHECK(nw <= kMaxWorkers) << "KVServerRowSyncHandle: a round merges at most " << kMaxWorkers << " workers, the job has "
                             << nw;
    Table();
    // kRowLookup / kRowErase (ps/row_handle.h): at once, as cmd 2; neither joins a round
    if (detail::ServeRowLifecycle("KVServerRowSyncHandle", st.table, req_meta, req_data, server, w)) return;
    const bool pooled = req_meta.push && (req_meta.cmd == kRowUpdatePooled || req_meta.cmd == kRowUpdatePooledStep);
    if (pooled) {
      CHECK(req_data.weights.empty())
          << "KVServerRowSyncHandle: a weighted pooled Push (cmd " << req_meta.cmd << ", KVWorker::ZPushPooledWeighted) "
          << "cannot join a round: a round's frames carry no weights (psg_table_update_pooled_merged has none)";
      CHECK(!req_data.offsets.empty()) << "KVServerRowSyncHandle: cmd " << req_meta.cmd
                                       << " needs the bag offsets of a pooled request (KVWorker::ZPushPooledAll)";
      CHECK_EQ((req_data.offsets.size() - 1) * w, req_data.vals.size())
          << "KVServerRowSyncHandle: a pooled Push carries width values per bag";
    } else if (req_meta.push) {
      CHECK_EQ(n * w, req_data.vals.size()) << "a Push carries width values per key";
      CHECK(req_meta.cmd >= 0 && req_meta.cmd <= kAccumulate) << "KVServerRowSyncHandle: unknown Push cmd " << req_meta.cmd;
    }
    if (!req_meta.push || req_meta.cmd == kAccumulate) {
      const int flags = (req_meta.push ? PSG_PUSH : 0) | (req_meta.pull ? PSG_PULL : 0);
      detail::ServeRows(req_meta, req_data, server, w, req_meta.push ? "server.handle.rows.push" : "server.handle.rows.pull",
                        [&](psg_stream s, const Key* keys, const float* vals, float* out) {
                          device::Check(psg_table_handle_any(st.table, flags, keys, vals, out, n, s),
                                        "psg_table_handle_any");
                        });
      return;
    }
    // a gradient Push: staged as detail::ServeRows stages it, then held
    Held h;
    h.meta = req_meta;
    h.keys = req_data.keys;
    h.vals = req_data.vals;
    if (pooled) {  // zero keys and nb > 0 bags is a frame like any other: its offsets are checked
      h.pooled = true;
      h.nb = req_data.offsets.size() - 1;
      h.offsets = req_data.offsets;
      h.doffsets = detail::ToDeviceAsync(req_data.offsets, dev);
      if (n) h.dkeys = detail::ToDeviceAsync(req_data.keys, dev);
      if (h.nb) h.dvals = detail::ToDeviceAsync(req_data.vals, dev);
    } else if (n) {
      h.dkeys = detail::ToDeviceAsync(req_data.keys, dev);
      h.dvals = detail::ToDeviceAsync(req_data.vals, dev);
      if (req_meta.pull) {
        h.dout = server->TakeDirectOut(n * w);
        h.direct = !h.dout.empty();
        if (!h.direct) h.dout = SVector<float>::OnDevice(n * w, dev);
      }
    }
    st.held.push_back(std::move(h));
    if ((int)st.held.size() == nw) Round(st, server);
  }

  int iteration() const { return state->iteration; }
  // New rows start from seeded uniform values in [lo, hi] (detail::RowInit, ps/row_handle.h)
  void SetInit(uint64_t seed, float lo, float hi) { state->init.Set("KVServerRowSyncHandle", state->table, seed, lo, hi); }
  // the rows the table holds now: a lookup leaves it as it is, an erase lowers it
  size_t size() const { return detail::RowTableSize(state->table); }

  // Rows, moments and the iteration to a file and back, as
  // KVServerRowOptHandle::SaveModel / LoadModel; between rounds only: a round
  // that is half gathered fails the CHECK.
  void SaveModel(const std::string& path) {
    CHECK(state->held.empty()) << "KVServerRowSyncHandle::SaveModel: " << state->held.size() << " Pushes of a round are held";
    SaveRowTable(Table(), state->iteration, path);
  }
  int LoadModel(const std::string& path) {
    CHECK(state->held.empty()) << "KVServerRowSyncHandle::LoadModel: " << state->held.size() << " Pushes of a round are held";
    return detail::LoadOwnRows(Table(), path, &state->iteration);
  }

 private:
  psg_table* Table() {
    return detail::EnsureRowTable(&state->table, PSG_F32, state->width, state->use_adam, state->lr, &state->init);
  }

  // LRServer.h:163-178: the update on the merged gradients, then every held answer
  static void Round(State& st, KVServer<float>* server) {
    const int k = (int)st.held.size();
    const int dev = PostOffice::Get()->device();
    const size_t w = st.width;
    bool pull = false, pooled = false, ends_iteration = false;
    for (const Held& h : st.held) {
      pull = pull || (h.meta.pull && h.keys.size());
      pooled = pooled || h.pooled;
      ends_iteration = ends_iteration || ((h.meta.cmd == 1 || h.meta.cmd == kRowUpdatePooledStep) &&
                                          h.meta.sender == PostOffice::WorkerRankToID(0));
    }
    if (pooled) {
      RoundPooled(st, k);
      Answer(st, server, ends_iteration);
      return;
    }
    std::vector<const uint64_t*> keys(k);
    std::vector<uint64_t> ns(k);
    std::vector<const float*> grads(k);
    std::vector<float*> outs(k);
    std::vector<SVector<float>> unread;  // the call answers every frame or none: replies nobody asked for
    for (int j = 0; j < k; ++j) {
      Held& h = st.held[j];
      ns[j] = h.keys.size();
      keys[j] = ns[j] ? h.dkeys.data() : nullptr;
      grads[j] = ns[j] ? h.dvals.data() : nullptr;
      outs[j] = h.dout.empty() ? nullptr : h.dout.data();
      if (pull && ns[j] && !outs[j]) {
        unread.push_back(SVector<float>::OnDevice(ns[j] * w, dev));
        outs[j] = unread.back().data();
      }
    }
    {
      stage::Scope t("server.handle.rows.round");
      device::Check(psg_table_update_merged(st.table, pull ? PSG_PUSH | PSG_PULL : PSG_PUSH, k, keys.data(), ns.data(),
                                            grads.data(), pull ? outs.data() : nullptr, st.lr, st.iteration,
                                            device::ThreadStream(), nullptr),
                    "psg_table_update_merged");
    }
    Answer(st, server, ends_iteration);
  }

  // A round that holds a pooled frame: the merged update over all k frames, then
  // the Pull of every held plain PushPull — the updated row for every occurrence.
  static void RoundPooled(State& st, int k) {
    std::vector<const uint64_t*> keys(k), offsets(k);
    std::vector<uint64_t> ns(k), nbs(k);
    std::vector<const float*> grads(k);
    for (int j = 0; j < k; ++j) {
      const Held& h = st.held[j];
      ns[j] = h.keys.size();
      nbs[j] = h.nb;
      keys[j] = ns[j] ? h.dkeys.data() : nullptr;
      offsets[j] = h.pooled ? h.doffsets.data() : nullptr;
      grads[j] = h.dvals.empty() ? nullptr : h.dvals.data();
    }
    stage::Scope t("server.handle.rows.round");
    device::Check(psg_table_update_pooled_merged(st.table, k, keys.data(), ns.data(), offsets.data(), nbs.data(),
                                                 grads.data(), st.lr, st.iteration, device::ThreadStream(), nullptr),
                  "psg_table_update_pooled_merged");
    for (const Held& h : st.held)
      if (!h.dout.empty())
        device::Check(psg_table_handle_any(st.table, PSG_PULL, h.dkeys.data(), nullptr, h.dout.data(), h.keys.size(),
                                           device::ThreadStream()),
                      "psg_table_handle_any");
  }

  static void Answer(State& st, KVServer<float>* server, bool ends_iteration) {
    if (ends_iteration) ++st.iteration;
    for (const Held& h : st.held) {
      KVPairs<float> res;
      if (h.meta.pull) {
        res.keys = h.keys;
        if (!h.direct) res.vals = h.keys.on_device() ? h.dout : detail::ToHost(h.dout);
      }
      // a deferred answer: Response() cannot know that the slice was written in place
      server->RunResponse(h.meta, res, h.direct);
    }
    st.held.clear();
  }
};

}  // namespace ps
