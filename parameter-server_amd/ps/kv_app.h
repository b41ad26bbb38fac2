// ps/kv_app.h — KVWorker / KVServer / KVServerDefaultHandle: the reference's
// KV app surface (src/ps/KVApp.h:27-458) over the MI355X data path.
//
// What runs where
//   worker  Push/Pull/PushPull build one request; the slicer cuts it by the
//           servers' key ranges — with std::lower_bound for host key arrays
//           (as KVApp.h:515-574) and with the psg_slice HIP kernel for key
//           arrays in HBM; one message per non-empty slice (frames zero-copy).
//   server  KVServerDefaultHandle keeps the value store in HBM (psg_store,
//           SORTED layout) and runs every request as the psg_store_handle
//           kernel.  HBM frames (a worker that holds its keys / values on a
//           GPU, or a host-vector request the worker staged into HBM,
//           detail::StageFrame) are read in place, over xGMI when the
//           worker's GPU is another one; host frames are copied into HBM.
//   merge   Pull replies are concatenated in key order: memcpy for host
//           replies (KVApp.h:713-720), the psg_merge kernel for HBM replies.
// Custom request handles registered with SetRequestHandle see host frames
// (HBM frames are copied to host first), exactly like the reference; a handle
// that can consume HBM frames registers with SetDeviceRequestHandle.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "internal/PostOffice.h"
#include "internal/customer.h"
#include "internal/device.h"
#include "internal/stage_time.h"
#include "ps/base.h"
#include "ps/range.h"
#include "ps/simple_app.h"
#include "ps/svector.h"

namespace ps {

/* keys (unique, ascending), vals, optional per-key value lengths (KVApp.h:27-37) */
template <typename Value>
struct KVPairs {
  SVector<Key> keys;
  SVector<Value> vals;
  SVector<int> lens;
  int priority = 0;
  // a pooled request (ZPullPooled / ZPushPooled): nb + 1 bag offsets into keys,
  // as psg_table_lookup_pooled takes them; empty on every other request
  SVector<uint64_t> offsets;
  // a weighted pooled request (ZPullPooledWeighted / ZPushPooledWeighted): one
  // f32 weight per key, whatever Value is; empty on every other request
  SVector<float> weights;
};

/* meta of one request (KVApp.h:42-57) */
struct KVMeta {
  int cmd;
  bool push;
  bool pull;
  int sender;
  int timestamp;
  int customer_id;
};

// The cmds of KVWorker's pooled calls, which the row handles serve
// (ps/row_handle.h, next to its kRowLookup = 3 and kRowErase = 4).
constexpr int kRowLookupPooled = 5;      // ZPullPooled
constexpr int kRowUpdatePooled = 6;      // ZPushPooled
constexpr int kRowUpdatePooledStep = 7;  // ZPushPooled(step): also ends worker 0's iteration
constexpr int kRowLookupPooledMean = 8;  // ZPullPooledMean to ONE server: the one-table mean

namespace detail {
template <typename T>
int DeviceOf(const std::vector<T>*) { return -1; }
template <typename T>
int DeviceOf(const SVector<T>* v) { return v->device(); }

/* host copy of an HBM array (no-op for host arrays) */
template <typename T>
SVector<T> ToHost(const SVector<T>& v) {
  if (!v.on_device() || v.empty()) return v;
  SVector<T> h = SVector<T>::Uninitialized(v.size());
  device::CopySync(h.data(), v.data(), v.size() * sizeof(T), 1);
  return h;
}
/* HBM copy of a host array on GPU dev (no-op for HBM arrays) */
template <typename T>
SVector<T> ToDevice(const SVector<T>& v, int dev) {
  if (v.on_device() || v.empty()) return v;
  SVector<T> d = SVector<T>::OnDevice(v.size(), dev);
  device::CopySync(d.data(), v.data(), v.size() * sizeof(T), 0);
  return d;
}
/* the same, enqueued on the thread stream without waiting (the caller's
 * later work on that stream is ordered after it; keep `v` alive until then) */
template <typename T>
SVector<T> ToDeviceAsync(const SVector<T>& v, int dev) {
  if (v.on_device() || v.empty()) return v;
  SVector<T> d = SVector<T>::OnDevice(v.size(), dev);
  device::Check(psg_memcpy(d.data(), v.data(), v.size() * sizeof(T), 0, device::ThreadStream()),
                "psg_memcpy H2D");
  return d;
}
// The copy a host-vector Push / Pull makes of the caller's array
// (KVApp.h:119-121, 155).  On a node with a GPU, once every server has
// answered that its handle takes HBM frames (Meta::hbm_handle: the default
// handle, SetDeviceRequestHandle), a large array (>= 4 MiB) is copied straight
// into HBM by the pipelined staging (device::StageToDevice): the request then
// takes the HBM path (device slicer, HBM frames, no H2D on the server) and the
// host copy overlaps the PCIe transfer.  Otherwise — a host handle such as
// test_kv_app_benchmark's, which would copy the frames back — or with
// PS_STAGE_TO_HBM=0, it is the reference's host SVector copy.
// PS_STAGE_MIN_BYTES moves the 4 MiB threshold (tests: the reference's
// test_kv_app.cpp, 10,000 keys, then runs its CHECKs on the HBM path —
// device slicer, HBM frames — with its own host vectors).
template <typename T>
SVector<T> StageFrame(const std::vector<T>& v, bool servers_take_hbm) {
  static const bool on = [] {
    const char* e = std::getenv("PS_STAGE_TO_HBM");
    return !(e && std::atoi(e) == 0);
  }();
  static const size_t min_bytes = [] {
    const char* e = std::getenv("PS_STAGE_MIN_BYTES");
    return e ? (size_t)std::atoll(e) : (size_t(4) << 20);
  }();
  const int dev = PostOffice::Get()->device();
  if (!on || !servers_take_hbm || dev < 0 || v.empty() || v.size() * sizeof(T) < min_bytes) return SVector<T>(v);
  SVector<T> d = SVector<T>::OnDevice(v.size(), dev);
  device::StageToDevice(d.data(), v.data(), v.size() * sizeof(T));
  return d;
}
// The key-list hash of LR key caching: the std::hash<ps::SVector<uint64_t>>
// specialisation of tests/src/LRServer.h:11-29, which the reference worker
// also uses (LRWorker.h:214-219), restated so a server finds the list a
// worker names.  psg_key_list_hash computes the same on device keys.
inline uint64_t KeyListHash(const Key* keys, size_t n) {
  uint64_t seed = n;
  for (size_t i = 0; i < n; ++i) {
    uint64_t x = keys[i] + 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    seed ^= x ^ x >> 31;
  }
  return seed;
}

/* PS_PUSH_RUNS=0: a server handles every queued Push on its own, never a run
 * of them in one pass (A/B; KVServer::OnReceive). */
inline bool PushRunsOn() {
  static const bool on = [] {
    const char* e = std::getenv("PS_PUSH_RUNS");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}
/* PS_MIXED_RUNS=0: a run holds Pushes of one shape only, never the Pulls and
 * PushPulls of distinct senders queued with them (A/B; KVServer::OnReceive). */
inline bool MixedRunsOn() {
  static const bool on = [] {
    const char* e = std::getenv("PS_MIXED_RUNS");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}
/* PS_RUN_GATHER_US: how long a server waits for the requests of the senders
 * it has heard from lately to join a run (KVServer::OnReceive); default 120
 * (the reference benchmark's layout at ns = nw = 4 on one GPU: 477-487 GB/s
 * with no wait, 574-609 with 120 us, noisier past it:
 * profiles/r6_dropin_gather_sweep.txt); 0: a run holds what is queued when it
 * starts. */
inline int RunGatherMicros() {
  static const int us = [] {
    const char* e = std::getenv("PS_RUN_GATHER_US");
    return e ? std::atoi(e) : 120;
  }();
  return us;
}
/* PS_RUN_GATHER_AUTO=<cap µs> (default 0: off): the gather window follows how
 * long this server's recent runs took (at least PS_RUN_GATHER_US, at most the
 * cap) — a sender missing from a run is most likely waiting for another
 * server's run of about that length before it sends its next request. */
inline int RunGatherAutoCap() {
  static const int us = [] {
    const char* e = std::getenv("PS_RUN_GATHER_AUTO");
    return e ? std::atoi(e) : 0;
  }();
  return us;
}
/* PS_RUN_GATHER_ORDINAL (default 1): the gather waits only for the recent
 * senders that are behind the run — those this server has taken fewer
 * requests from than the run's lowest ordinal (its n-th request from each) —
 * and for up to PS_RUN_GATHER_ORD_US (default 1000) µs.  A sender that is not
 * behind has had this round's request served already and may itself wait for
 * this server's answer to another; one that is behind is held up only by
 * servers serving lower ordinals, so the waits form no cycle.  0: wait for
 * every recent sender for PS_RUN_GATHER_US (A/B). */
inline bool RunGatherOrdinal() {
  static const bool on = [] {
    const char* e = std::getenv("PS_RUN_GATHER_ORDINAL");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}
inline int RunGatherOrdMicros() {
  static const int us = [] {
    const char* e = std::getenv("PS_RUN_GATHER_ORD_US");
    return e ? std::atoi(e) : 1000;
  }();
  return us;
}
/* PS_TRACE_REQUESTS=<file>: every request a KVServer hands to its handle is
 * appended to <file> as one line "server sender timestamp push pull keys
 * run_size run_pos" (run_size 1 for a request handled on its own) — the
 * arrival order a test replays through the oracle.  One write(2) per line on
 * an O_APPEND descriptor, so the servers of a job may share the file. */
inline void TraceRequest(int server, const KVMeta& m, size_t keys, size_t run_size, size_t run_pos) {
  static const int fd = [] {
    const char* e = std::getenv("PS_TRACE_REQUESTS");
    return e && *e ? ::open(e, O_WRONLY | O_CREAT | O_APPEND, 0644) : -1;
  }();
  if (fd < 0) return;
  char line[160];
  const int len = std::snprintf(line, sizeof(line), "%d %d %d %d %d %zu %zu %zu\n", server, m.sender, m.timestamp,
                                (int)m.push, (int)m.pull, keys, run_size, run_pos);
  if (len > 0) (void)!::write(fd, line, (size_t)len);
}

/* A worker sends an HBM key list it sliced before on the bounds it had then,
 * unconfirmed, when every server checks its slices (KVWorker::Send);
 * PS_SPEC_SLICE=0: every request is sliced first (A/B). */
inline bool SpecSliceOn() {
  static const bool on = [] {
    const char* e = std::getenv("PS_SPEC_SLICE");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}
/* PS_TRACE_GATHER=<file> (diagnostics): one line per gathered run, "server
 * head_sender head_ordinal run_size why waited_us" — why the gather ended:
 * 0 run full, 1 no sender behind (or no window), 2 a queued message that
 * may not join, 3 the window timed out. */
inline void TraceGather(int server, int sender, uint64_t ordinal, size_t size, int why, double us) {
  static const int fd = [] {
    const char* e = std::getenv("PS_TRACE_GATHER");
    return e && *e ? ::open(e, O_WRONLY | O_CREAT | O_APPEND, 0644) : -1;
  }();
  if (fd < 0) return;
  char line[128];
  const int len = std::snprintf(line, sizeof(line), "%d %d %llu %zu %d %.1f\n", server, sender,
                                (unsigned long long)ordinal, size, why, us);
  if (len > 0) (void)!::write(fd, line, (size_t)len);
}

/* ZPull offers the servers its HBM output (Meta::direct_reply); PS_DIRECT_REPLY=0
 * turns the offer off (A/B): every reply is then merged by psg_merge. */
inline bool DirectReplyOn() {
  static const bool on = [] {
    const char* e = std::getenv("PS_DIRECT_REPLY");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}
}  // namespace detail

template <typename Value>
struct KVServerDefaultHandle;

template <typename Value>
class KVWorker : public SimpleApp {
 public:
  using Data = KVPairs<Value>;
  using Callback = std::function<void()>;
  using SlicedKVs = std::vector<std::pair<bool, Data>>;
  using Slicer = std::function<void(Data& send, const std::vector<Range>& ranges, SlicedKVs* sliced)>;

  KVWorker(int app_id, int customer_id) : SimpleApp() {
    slicer_ = [this](Data& send, const std::vector<Range>& ranges, SlicedKVs* sliced) {
      DefaultSlicer(send, ranges, sliced);
    };
    app_id_ = app_id;
    customer_ = new Customer(app_id, customer_id, [this](const Message& m) { OnReceive(m); });
  }
  ~KVWorker() override {
    delete customer_;
    customer_ = nullptr;
  }

  /* KVApp.h:112-122: the vectors are copied into SVectors (into HBM on a
   * node with a GPU, detail::StageFrame; the lens stay on the host) */
  int Push(const std::vector<Key>& keys, const std::vector<Value>& vals,
           const std::vector<int>& lens = {}, int cmd = 0, const Callback& cb = nullptr,
           int priority = 0) {
    if (!lens.empty()) return ZPush(SVector<Key>(keys), SVector<Value>(vals), SVector<int>(lens), cmd, cb, priority);
    const bool hbm = servers_take_hbm_.load();
    SVector<Key> skeys;
    SVector<Value> svals;
    {
      stage::Scope t("worker.push.copy", keys.size() * sizeof(Key) + vals.size() * sizeof(Value));
      skeys = detail::StageFrame(keys, hbm);
      svals = detail::StageFrame(vals, hbm);
    }
    return ZPush(skeys, svals, SVector<int>(), cmd, cb, priority);
  }

  /* KVApp.h:148-162 */
  int Pull(const std::vector<Key>& keys, std::vector<Value>* vals, std::vector<int>* lens = nullptr,
           int cmd = 0, const Callback& cb = nullptr, int priority = 0) {
    SVector<Key> skeys;
    {
      stage::Scope t("worker.pull.copy_keys", keys.size() * sizeof(Key));
      skeys = lens ? SVector<Key>(keys) : detail::StageFrame(keys, servers_take_hbm_.load());
    }
    int ts = AddPullCB(skeys, vals, lens, cmd, cb);
    Data kvs;
    kvs.keys = skeys;
    kvs.priority = priority;
    Send(ts, false, true, cmd, kvs);
    return ts;
  }

  /* KVApp.h:188-213 */
  int PushPull(const std::vector<Key>& keys, const std::vector<Value>& vals, std::vector<Value>* outs,
               std::vector<int>* lens = nullptr, int cmd = 0, const Callback& cb = nullptr,
               int priority = 0) {
    CHECK_NOTNULL(outs);
    if (outs->empty())
      outs->resize(vals.size());
    else
      CHECK_EQ(vals.size(), outs->size());
    const bool hbm = servers_take_hbm_.load();
    SVector<Key> skeys = lens ? SVector<Key>(keys) : detail::StageFrame(keys, hbm);
    SVector<Value> svals = lens ? SVector<Value>(vals) : detail::StageFrame(vals, hbm);
    auto souts = new SVector<Value>(outs->data(), outs->size());
    SVector<int>* slens = lens ? new SVector<int>(lens->data(), lens->size()) : nullptr;
    return ZPushPull(skeys, svals, souts, slens, cmd,
                     [souts, slens, cb]() {
                       delete souts;
                       delete slens;
                       if (cb) cb();
                     },
                     priority);
  }

  void Wait(int timestamp) override { customer_->WaitRequest(timestamp); }

  /* zero-copy forms (KVApp.h:234-291); SVectors may live in HBM */
  int ZPush(const SVector<Key>& keys, const SVector<Value>& vals, const SVector<int>& lens = {},
            int cmd = 0, const Callback& cb = nullptr, int priority = 0) {
    int ts = customer_->NewRequest(kServerGroup);
    AddCallback(ts, cb);
    Data kvs;
    kvs.keys = keys;
    kvs.vals = vals;
    kvs.lens = lens;
    kvs.priority = priority;
    Send(ts, true, false, cmd, kvs);
    return ts;
  }
  int ZPull(const SVector<Key>& keys, SVector<Value>* vals, SVector<int>* lens = nullptr, int cmd = 0,
            const Callback& cb = nullptr, int priority = 0) {
    int ts = AddPullCB(keys, vals, lens, cmd, cb);
    Data kvs;
    kvs.keys = keys;
    kvs.priority = priority;
    // HBM keys and a sized HBM output, no lens: offer each server its slice of
    // the output (the request's vals frame), so a handle that can write its
    // reply there does, and the merge copy disappears (detail::DirectReply)
    const bool direct = vals && lens == nullptr && keys.on_device() && keys.size() && vals->on_device() &&
                        vals->size() && vals->size() % keys.size() == 0 && detail::DirectReplyOn();
    if (direct) kvs.vals = *vals;
    Send(ts, false, true, cmd, kvs, direct);
    return ts;
  }
  int ZPushPull(const SVector<Key>& keys, const SVector<Value>& vals, SVector<Value>* outs,
                SVector<int>* lens = nullptr, int cmd = 0, const Callback& cb = nullptr,
                int priority = 0) {
    int ts = AddPullCB(keys, outs, lens, cmd, cb);
    Data kvs;
    kvs.keys = keys;
    kvs.vals = vals;
    kvs.priority = priority;
    if (lens) kvs.lens = *lens;  // the reference forwards the output lens (KVApp.h:287-288)
    // as ZPull: offer each server its slice of the HBM output (outs mirrors vals)
    const bool direct = outs && lens == nullptr && keys.on_device() && keys.size() && outs->on_device() &&
                        outs->size() == vals.size() && vals.on_device() && detail::DirectReplyOn();
    Send(ts, true, true, cmd, kvs, direct, direct ? outs : nullptr);
    return ts;
  }

  /* ---- key lists in any order and with repeats ----------------------------------
   * The calls above cut a request by lower_bound (DefaultSlicer, KVApp.h:515-574),
   * which presumes ascending keys.  These six take a minibatch's id list as it
   * is — any order, hot ids named many times — and route it: the list's stable
   * partition by owning server (psg_route), so every server gets its keys in
   * arrival order, and every reply row goes back to the position its key had
   * in the caller's list.  With servers whose handle serves such lists (the row
   * handles built with any_order, KVServerRowSyncHandle) the result is, bit for
   * bit, that of one server over the whole key range serving the whole list.
   * Arguments as the namesake's, without lens (rows have one width).  CHECKs:
   * no custom slicer is installed (routing presumes range ownership); vals and
   * the output hold a multiple of keys.size() values.
   *
   * Z forms: keys, vals and the output live in HBM.  One server: the list goes
   * on whole, as ZPush / ZPull / ZPushPull send it.  A list already partitioned
   * by owner (every sorted list) is sent from the caller's own arrays on the
   * bounds psg_route returned — one extra pass over the keys, no copy.  Any
   * other list: pooled HBM frames take the routed keys, perm and the gathered
   * values (psg_rows_gather); each server is sent its stretch on psg_route's
   * exact bounds (no slicer kernel, no hint, no unconfirmed slice); a Pull's
   * replies land in a routed output frame, offered to the servers for direct
   * reply as ZPull offers its output; when the last reply is in,
   * psg_rows_scatter puts the rows at the caller's positions, the frames go
   * back to the pool, and then the callback runs.  Wait(ts) returns after that. */
  int ZPushAny(const SVector<Key>& keys, const SVector<Value>& vals, int cmd = 0, const Callback& cb = nullptr,
               int priority = 0) {
    return SendAny(keys, &vals, nullptr, cmd, cb, priority);
  }
  int ZPullAny(const SVector<Key>& keys, SVector<Value>* vals, int cmd = 0, const Callback& cb = nullptr,
               int priority = 0) {
    CHECK_NOTNULL(vals);
    return SendAny(keys, nullptr, vals, cmd, cb, priority);
  }
  int ZPushPullAny(const SVector<Key>& keys, const SVector<Value>& vals, SVector<Value>* outs, int cmd = 0,
                   const Callback& cb = nullptr, int priority = 0) {
    CHECK_NOTNULL(outs);
    CHECK_EQ(vals.size(), outs->size()) << "ZPushPullAny: the output mirrors vals";
    return SendAny(keys, &vals, outs, cmd, cb, priority);
  }
  /* ---- bags of ids on a table sharded over the servers ---------------------------
   * keys: n ids in any order and with repeats; offsets: nb + 1 words, bag b is
   * keys[offsets[b] .. offsets[b+1]) (the rules of psg_table_lookup_pooled); all
   * in HBM.  The list is routed as the Any calls route it (a list already
   * partitioned by owner is sent from the caller's own keys), psg_route_bags
   * cuts every bag into the servers' shares, and every server that owns ids is
   * sent its stretch of keys and its nb + 1 offsets, for the row handles' cmds
   * kRowLookupPooled / kRowUpdatePooled / kRowUpdatePooledStep (ps/row_handle.h).
   * The definition is include/psg.h's ("Bags across servers").
   * ZPullPooled: out holds nb * k values.  Each server is offered its own
   *   nb * k frame from the HBM pool; when the last reply is in, psg_pool_reduce
   *   adds the frames in rank order into out, the frames go back to the pool,
   *   and then the callback runs; Wait(ts) returns after that.  One server: out
   *   itself is offered and nothing is reduced.  nb * k values per server come
   *   back instead of ZPullAny's n * k in all: fewer bytes when bags hold more
   *   ids than there are servers.
   * ZPushPooled: grads holds nb * k values, one gradient row per bag; every
   *   server gets the whole frame.  step: the update also ends worker 0's
   *   iteration on the servers it reaches, as a Push with cmd 1 does.
   * ZPushPooledAll: ZPushPooled with one difference: EVERY server is sent a
   *   message.  A server that owns none of the ids gets zero keys, its nb + 1
   *   offsets (psg_route_bags writes them for it: all zero) and the gradient
   *   frame.  It is the call of a sync job (KVServerRowSyncHandle): a server
   *   closes its round when num_workers() gradient Pushes are held, so in a sync
   *   job every worker's Push must reach every server — the rule the plain
   *   calls have as well (ZPushAny sends nothing to a server that owns no key of
   *   the list: there a worker's list has to reach every server).  ZPushPooled
   *   skips the servers that own none of a list's ids, and their rounds would
   *   wait for ever.
   * CHECKs: no custom slicer; out / grads hold a multiple of nb values;
   * psg_route_bags did not refuse the offsets (nothing is sent then). */
  int ZPullPooled(const SVector<Key>& keys, const SVector<uint64_t>& offsets, SVector<Value>* out,
                  const Callback& cb = nullptr, int priority = 0) {
    CHECK_NOTNULL(out);
    return SendPooled(keys, offsets, nullptr, out, false, false, cb, priority);
  }
  int ZPushPooled(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>& grads,
                  bool step = false, const Callback& cb = nullptr, int priority = 0) {
    return SendPooled(keys, offsets, &grads, nullptr, step, false, cb, priority);
  }
  int ZPushPooledAll(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>& grads,
                     bool step = false, const Callback& cb = nullptr, int priority = 0) {
    return SendPooled(keys, offsets, &grads, nullptr, step, true, cb, priority);
  }
  /* ---- the other two poolings of a bag: per-id weights, and the mean ----------------
   * The definitions are include/psg.h's ("Weighted and mean bags across servers").
   * weights: n floats in HBM, one per position of keys (f32 whatever Value is).
   * ZPullPooledWeighted / ZPushPooledWeighted: ZPullPooled / ZPushPooled with the
   *   weights routed like the keys (psg_rows_gather on a permuted route, the
   *   caller's own array on an identity route); every server that owns ids gets
   *   its stretch of them as one more frame (Meta::weighted) and serves its share
   *   with psg_table_lookup_pooled_weighted / _update_pooled_weighted(PSG_POOL_SUM).
   * ZPullPooledMean: one server: cmd kRowLookupPooledMean with out offered, the
   *   one-table mean bit for bit.  Several: the servers answer plain SUM partials
   *   (cmd kRowLookupPooled) and, when the last reply is in, psg_pool_reduce_mean
   *   folds them and divides once by the bag lengths of the CALLER's offsets
   *   (also when one server owns every id).  No owners: out is +0.
   * ZPushPooledMean / ZPushPooledMeanAll: psg_pool_scale_mean divides the nb
   *   gradient rows once into a pooled frame, which goes the way ZPushPooled /
   *   ZPushPooledAll send grads: a mean Push is a plain pooled Push to the
   *   servers, sync-mode rounds included.
   * CHECKs: what the unweighted calls CHECK; weights.size() == n and weights in
   * HBM; the weighted and the mean Pushes need Value == float (the table's update
   * is F32 only). */
  int ZPullPooledWeighted(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<float>& weights,
                          SVector<Value>* out, const Callback& cb = nullptr, int priority = 0) {
    CHECK_NOTNULL(out);
    return SendPooled(keys, offsets, nullptr, out, false, false, cb, priority, &weights);
  }
  int ZPushPooledWeighted(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<float>& weights,
                          const SVector<Value>& grads, bool step = false, const Callback& cb = nullptr,
                          int priority = 0) {
    return SendPooled(keys, offsets, &grads, nullptr, step, false, cb, priority, &weights);
  }
  int ZPullPooledMean(const SVector<Key>& keys, const SVector<uint64_t>& offsets, SVector<Value>* out,
                      const Callback& cb = nullptr, int priority = 0) {
    CHECK_NOTNULL(out);
    return SendPooled(keys, offsets, nullptr, out, false, false, cb, priority, nullptr, true);
  }
  int ZPushPooledMean(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>& grads,
                      bool step = false, const Callback& cb = nullptr, int priority = 0) {
    return SendPooled(keys, offsets, &grads, nullptr, step, false, cb, priority, nullptr, true);
  }
  int ZPushPooledMeanAll(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>& grads,
                         bool step = false, const Callback& cb = nullptr, int priority = 0) {
    return SendPooled(keys, offsets, &grads, nullptr, step, true, cb, priority, nullptr, true);
  }
  /* Host-vector forms: the same routing done on the host (a stable counting
   * pass over the owners), the routed copies sent as host frames on its bounds,
   * the replies un-permuted on the host in the callback.  A correctness path,
   * not a fast one: every value is copied twice by one thread. */
  int PushAny(const std::vector<Key>& keys, const std::vector<Value>& vals, int cmd = 0, const Callback& cb = nullptr,
              int priority = 0) {
    return SendAnyHost(keys, &vals, nullptr, cmd, cb, priority);
  }
  int PullAny(const std::vector<Key>& keys, std::vector<Value>* vals, int cmd = 0, const Callback& cb = nullptr,
              int priority = 0) {
    CHECK_NOTNULL(vals);
    return SendAnyHost(keys, nullptr, vals, cmd, cb, priority);
  }
  int PushPullAny(const std::vector<Key>& keys, const std::vector<Value>& vals, std::vector<Value>* outs, int cmd = 0,
                  const Callback& cb = nullptr, int priority = 0) {
    CHECK_NOTNULL(outs);
    if (outs->empty())
      outs->resize(vals.size());
    else
      CHECK_EQ(vals.size(), outs->size());
    return SendAnyHost(keys, &vals, outs, cmd, cb, priority);
  }

  /* slices its servers refused (Refused; PS_SPEC_SLICE) */
  uint64_t refused_slices() const { return refused_.load(); }
  void set_slicer(const Slicer& slicer) {
    default_slicer_ = false;
    CHECK(static_cast<bool>(slicer));
    slicer_ = slicer;
  }

 private:
  struct Reply {
    Data kv;
    int sender;
    bool direct = false;  // the server wrote the values into the output in place
  };
  // servers whose replies said their handle takes HBM frames
  void NoteHbmServer(int sender) {
    std::lock_guard<std::mutex> lk(mu_);
    const int ns = PostOffice::Get()->num_servers();
    if (hbm_server_.size() != (size_t)ns) hbm_server_.assign(ns, 0);
    const int r = PostOffice::IDToRank(sender);
    if (r < ns && !hbm_server_[r]) {
      hbm_server_[r] = 1;
      if (++hbm_count_ == ns) servers_take_hbm_ = true;
    }
  }
  std::vector<char> hbm_server_;
  int hbm_count_ = 0;
  std::atomic<bool> servers_take_hbm_{false};
  // servers whose handle takes unconfirmed slices (Meta::spec_slice in their
  // replies); all of them: the worker may send the slicer's hints unconfirmed
  void NoteSpecServer(int sender) {
    std::lock_guard<std::mutex> lk(mu_);
    const int ns = PostOffice::Get()->num_servers();
    if (spec_server_.size() != (size_t)ns) spec_server_.assign(ns, 0);
    const int r = PostOffice::IDToRank(sender);
    if (r < ns && !spec_server_[r]) {
      spec_server_[r] = 1;
      if (++spec_count_ == ns) servers_take_spec_ = true;
    }
  }
  std::vector<char> spec_server_;
  int spec_count_ = 0;
  std::atomic<bool> servers_take_spec_{false};
  // a request sent on unconfirmed slices: what a refusal needs to re-send
  struct SpecSend {
    bool push = false, pull = false, direct = false, has_outs = false;
    int cmd = 0;
    Data kvs;
    SVector<Value> outs;
    std::vector<uint64_t> pos;  // the hinted key bounds, num_servers + 1
  };
  std::unordered_map<int, SpecSend> spec_sends_;
  std::unordered_map<const void*, bool> spec_stale_;  // key arrays a refusal proved re-sliced since
  bool default_slicer_ = true;
  std::atomic<uint64_t> refused_{0};
  void SendOne(int timestamp, bool push, bool pull, int cmd, int priority, const Data& whole, const Data& kv,
               bool direct, const SVector<Value>* outs, int server_rank, bool spec);
  void Refused(const Message& msg);
  void SendPieces(int timestamp, const SpecSend& sp, uint64_t a, uint64_t b, const std::vector<uint64_t>& pos,
                  int* sent);

  void AddCallback(int timestamp, const Callback& cb) {
    if (!cb) return;
    std::lock_guard<std::mutex> lk(mu_);
    callbacks_[timestamp] = cb;
  }
  void RunCallback(int timestamp);
  void Send(int timestamp, bool push, bool pull, int cmd, const Data& kvs, bool direct = false,
            const SVector<Value>* outs = nullptr);
  /* the slices of a request to their servers (Send, SendBounds) */
  void SendSliced(int timestamp, bool push, bool pull, int cmd, const Data& kvs, SlicedKVs& sliced, bool direct,
                  const SVector<Value>* outs, bool spec);
  /* Send on key bounds known exactly (a routed list): pos[i] .. pos[i + 1] is
   * server i's stretch.  No slicer, no hint, no unconfirmed slice. */
  void SendBounds(int timestamp, bool push, bool pull, int cmd, const Data& kvs, const std::vector<uint64_t>& pos,
                  bool direct, const SVector<Value>* outs);
  /* the Z and host forms of the any-order calls: vals == nullptr: no Push,
   * outs == nullptr: no Pull */
  int SendAny(const SVector<Key>& keys, const SVector<Value>* vals, SVector<Value>* outs, int cmd, const Callback& cb,
              int priority);
  int SendAnyHost(const std::vector<Key>& keys, const std::vector<Value>* vals, std::vector<Value>* outs, int cmd,
                  const Callback& cb, int priority);
  /* ZPullPooled (grads == nullptr) and ZPushPooled / ZPushPooledAll (out ==
   * nullptr; all: also the servers that own none of the ids are sent to);
   * weights != nullptr: the Weighted calls; mean: the Mean calls */
  int SendPooled(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>* grads,
                 SVector<Value>* out, bool step, bool all, const Callback& cb, int priority,
                 const SVector<float>* weights = nullptr, bool mean = false);
  void OnReceive(const Message& msg) override;
  void DefaultSlicer(Data& send, const std::vector<Range>& ranges, SlicedKVs* sliced);
  /* routed: the request went out on SendBounds — its keys are partitioned by
   * owner, not sorted: replies are ordered by server, not looked up by key */
  template <typename C, typename D>
  int AddPullCB(const SVector<Key>& keys, C* vals, D* lens, int cmd, const Callback& cb, bool routed = false);
  template <typename C, typename D>
  void MergePull(const SVector<Key>& keys, std::vector<Reply>& kvs, C* vals, D* lens, bool routed = false);

  std::unordered_map<int, std::vector<Reply>> recv_kvs_;
  std::unordered_map<int, Callback> callbacks_;
  std::mutex mu_;
  Slicer slicer_;
};

/* one request of a run of queued requests (KVServer::OnReceive) */
template <typename Value>
struct KVRunItem {
  KVMeta meta;
  KVPairs<Value> data;
  SVector<Value> out;  // the output slice a Pull offered for its reply (direct reply), else empty
  bool spec = false;   // its slice is the worker's unconfirmed hint (Meta::spec_slice)
};

template <typename Value>
class KVServer : public SimpleApp {
 public:
  using ReqHandle = std::function<void(const KVMeta& req_meta, const KVPairs<Value>& req_data, KVServer* server)>;
  /* A run of requests queued one behind the other (see OnReceive), in arrival
   * order; the handle answers every one of them. */
  using RunHandle = std::function<void(std::vector<KVRunItem<Value>>& run, KVServer* server)>;
  static constexpr int kMaxRun = 16;  // requests a run holds at most (psg_store_run)

  explicit KVServer(int app_id) : SimpleApp() {
    app_id_ = app_id;
    customer_ = new Customer(app_id, app_id, [this](const Message& m) { OnReceive(m); });
  }
  ~KVServer() override {
    delete customer_;
    customer_ = nullptr;
  }

  /* a host handle: sees host frames (KVApp.h:405-408) */
  void SetRequestHandle(const ReqHandle& request_handle) {
    CHECK(static_cast<bool>(request_handle)) << "invalid request handle";
    Install(request_handle, false);
  }
  /* the default handle keeps its store in HBM and takes frames where they are,
   * and serves a run of queued Pushes on one key list in one pass */
  void SetRequestHandle(const KVServerDefaultHandle<Value>& h) {
    Install(h, true, [hd = h](std::vector<KVRunItem<Value>>& run, KVServer* server) mutable { hd.Run(run, server); });
  }
  /* a handle that consumes HBM frames itself */
  void SetDeviceRequestHandle(const ReqHandle& request_handle) {
    CHECK(static_cast<bool>(request_handle)) << "invalid request handle";
    Install(request_handle, true);
  }

  /* reply to a request (KVApp.h:491-513); frames may be host or HBM */
  void Response(const KVMeta& req, const KVPairs<Value>& res = KVPairs<Value>());
  /* For a run handle: reply to one request of a run; `direct` says the handle
   * wrote the Pull's values into the output slice the request offered
   * (KVRunItem::out), so the reply carries its keys and no values. */
  void RunResponse(const KVMeta& req, const KVPairs<Value>& res, bool direct) { Reply(req, res, direct); }
  /* For a run handle: refuse a request whose unconfirmed slice (KVRunItem::spec)
   * holds a key outside this server's range — nothing of it was applied; the
   * worker re-sends its keys sliced for real. */
  void RunRefuse(const KVMeta& req) { Reply(req, KVPairs<Value>(), false, true); }
  /* this server takes unconfirmed slices: its handle checks every key of a run
   * against its own range and refuses a wrong slice instead of failing */
  bool TakesSpecSlices() const {
    return static_cast<bool>(run_handle_) && device_frames_.load() && detail::PushRunsOn() && detail::MixedRunsOn();
  }
  /* For a run handle: serve one request of a run with the installed handle, as
   * if it had been taken on its own (its output offer included). */
  void ServeOne(const KVRunItem<Value>& item) {
    direct_out_ = item.out;
    direct_ts_ = item.meta.timestamp;
    direct_sender_ = item.meta.sender;
    direct_taken_ = false;
    request_handle_(item.meta, item.data, this);
    direct_out_ = SVector<Value>();
    direct_taken_ = false;
  }

 private:
  void OnReceive(const Message& msg) override;
  void Reply(const KVMeta& req, const KVPairs<Value>& res, bool direct, bool refused = false);
  void Install(const ReqHandle& h, bool device_frames, const RunHandle& run = nullptr) {
    {
      std::lock_guard<std::mutex> lk(handle_mu_);
      request_handle_ = h;
      run_handle_ = run;
      device_frames_ = device_frames;
    }
    handle_cv_.notify_all();
  }
  /* a request a run may hold: a Push, Pull or PushPull with keys and no lens
   * ([keys, vals], [keys, out] for a Pull offering its output, [keys, vals, out]
   * for such a PushPull) */
  static bool PlainRequest(const Message& m) {
    if (!m.meta.request || m.meta.simple_app || m.meta.control.cmd != Control::EMPTY) return false;
    if (!(m.meta.push || m.meta.pull) || m.meta.bags) return false;
    const size_t want = (m.meta.direct_reply && m.meta.push && m.meta.pull) ? 3 : 2;
    return m.data.size() == want && m.data[0].size() > 0 && (!m.meta.push || m.data[1].size() > 0);
  }
  static KVMeta MetaOf(const Message& msg) {
    KVMeta meta;
    meta.cmd = msg.meta.head;
    meta.push = msg.meta.push;
    meta.pull = msg.meta.pull;
    meta.sender = msg.meta.sender;
    meta.timestamp = msg.meta.timestamp;
    meta.customer_id = msg.meta.customer_id;
    return meta;
  }
  RunHandle run_handle_;
  // the senders of the last requests this server took (the gather window's
  // target: how many requests one step brings), a ring of 64
  int recent_[64] = {};
  unsigned recent_n_ = 0;
  int gather_idle_ = 0;  // gather windows in a row that timed out with nothing gained
  int gather_cool_ = 0;  // requests left to take without a window
  double run_us_ = 0;    // this server's recent run times (moving average, µs)
  // requests taken from each sender so far (a request's ordinal: the n-th from
  // its sender)
  std::unordered_map<int, uint64_t> taken_;
  // senders a window timed out waiting for: not waited for again until they
  // send (a worker that skips this server, or has stopped)
  std::unordered_map<int, bool> stalled_;
  uint64_t Take(int sender) {
    stalled_.erase(sender);
    return ++taken_[sender];
  }
  // a recent sender outside the run that this server has taken fewer than m
  // requests from (its next request is the run's round or an earlier one);
  // mark: note every such sender as stalled instead
  bool SendersBehind(const std::vector<KVRunItem<Value>>& items, uint64_t m, bool mark = false) {
    const unsigned n = recent_n_ < 64 ? recent_n_ : 64;
    bool any = false;
    for (unsigned i = 0; i < n; ++i) {
      const int w = recent_[i];
      bool in = false;
      for (const auto& it : items) in = in || it.meta.sender == w;
      if (in || stalled_.count(w)) continue;
      auto t = taken_.find(w);
      if ((t == taken_.end() ? 0 : t->second) < m) {
        if (!mark) return true;
        stalled_[w] = true;
        any = true;
      }
    }
    return any;
  }
  void NoteSender(int sender) { recent_[recent_n_++ & 63] = sender; }
  size_t RecentSenders(int sender) {
    NoteSender(sender);
    const unsigned n = recent_n_ < 64 ? recent_n_ : 64;
    int seen[64];
    size_t c = 0;
    for (unsigned i = 0; i < n; ++i) {
      bool dup = false;
      for (size_t j = 0; j < c && !dup; ++j) dup = seen[j] == recent_[i];
      if (!dup) seen[c++] = recent_[i];
    }
    return c < (size_t)kMaxRun ? c : (size_t)kMaxRun;
  }
  // The customer thread may receive a request before the program installs its
  // handle (it is created with the KVServer); it waits for the handle instead
  // of failing the reference's CHECK (KVApp.h:487) on that race.
  ReqHandle request_handle_;
  std::atomic<bool> device_frames_{false};
  std::mutex handle_mu_;
  std::condition_variable handle_cv_;
  // the output slice a direct-reply Pull offers while its handle runs (the
  // customer thread runs one handle at a time), and whether the handle took it
  // (atomics: a handle may answer a deferred request from another thread)
  SVector<Value> direct_out_;
  std::atomic<int> direct_ts_{-1}, direct_sender_{-1};
  std::atomic<bool> direct_taken_{false};

 public:
  /* For a handle that answers a Pull from HBM: the caller's output slice for
   * this request's values when the worker offered one of n values (ZPull
   * with HBM keys and a sized HBM output), else an empty SVector.  A handle
   * that takes it must write the reply values there (ordered before its
   * Response) and then Response with keys and no values, from inside the
   * handle (a deferred Response is not marked as written in place). */
  SVector<Value> TakeDirectOut(size_t n) {
    if (direct_out_.size() != n || !direct_out_.on_device()) return SVector<Value>();
    direct_taken_ = true;
    return direct_out_;
  }
};

/* The default handle (KVApp.h:433-458): `store[key] += val` for a push,
 * `res.vals[i] = store[key]` (post-update) for a pull, absent keys inserted
 * with 0 — with the store in HBM (psg_store, SORTED) and the loop as HIP
 * kernels per request.  One value per key (the reference's CHECK at :441).
 *
 * KVServerDefaultHandle<V>(true) also serves the key-cache protocol of the
 * reference's LR server (LRServer.h:127-142) on this store: a request with
 * more than one key is handled as usual and its key list is cached under its
 * hash (detail::KeyListHash / psg_key_list_hash), resolved once to store
 * slots; a request with ONE key names a cached list by that hash and runs on
 * the cached slots (psg_store_handle_slots: 16 B / key for a Push instead of
 * a validation pass plus the resolve).  The slots are re-resolved after the
 * store inserts keys.  As in the reference, a one-key request is then always
 * read as a hash, and every list should go to one server (LR_ps runs ns = 1). */
template <typename Value>
struct KVServerDefaultHandle {
  struct Cached {
    SVector<Key> keys;        // the list (HBM), kept for a re-resolve
    SVector<uint32_t> slots;  // its store slots (HBM)
    uint64_t store_size = 0;  // the store's size when resolved (an insert moves slots)
    // the first slot when the slots are a stretch of the store (the list covers
    // its range: LRServer.h:144's every-feature list), else UINT64_MAX: then a
    // request needs no slot stream (psg_store_handle_stretch)
    uint64_t stretch = UINT64_MAX;
  };
  struct State {
    psg_store* store = nullptr;
    bool key_cache = false;
    std::unordered_map<uint64_t, Cached> cache;
    ~State() {
      if (store) psg_store_destroy(store);
    }
  };
  std::shared_ptr<State> state = std::make_shared<State>();

  explicit KVServerDefaultHandle(bool use_key_cache = false) { state->key_cache = use_key_cache; }

  void operator()(const KVMeta& req_meta, const KVPairs<Value>& req_data, KVServer<Value>* server) {
    size_t n = req_data.keys.size();
    KVPairs<Value> res;
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerDefaultHandle: the value store lives in HBM and this node has no GPU";
    constexpr int dt = device::DType<Value>();
    CHECK_GE(dt, 0) << "KVServerDefaultHandle: value type not supported by the HBM store";
    if (!state->store)
      device::Check(psg_store_create(PSG_STORE_SORTED, dt, 0, kMaxKey, 0, &state->store), "psg_store_create");
    const bool on_dev = req_data.keys.on_device();
    const int flags = (req_meta.push ? PSG_PUSH : 0) | (req_meta.pull ? PSG_PULL : 0);
    psg_stream s = device::ThreadStream();
    SVector<Value> dout;
    bool direct = false;
    if (state->key_cache && n == 1 && flags) {
      // a cached list named by its hash (LRServer.h:129-135)
      Key h = 0;
      if (on_dev) device::CopySync(&h, req_data.keys.data(), sizeof(Key), 1);
      else h = req_data.keys[0];
      auto it = state->cache.find(h);
      CHECK(it != state->cache.end()) << "Keys don't exist with hash value: " << h;
      Cached& c = it->second;
      n = c.keys.size();
      if (req_meta.push) CHECK_EQ(n, req_data.vals.size());
      Refresh(c, s);
      SVector<Value> dvals;
      if (req_meta.push) dvals = detail::ToDeviceAsync(req_data.vals, dev);
      if (req_meta.pull) dout = PullOutput(server, n, dev, &direct);
      if (c.stretch != UINT64_MAX)
        device::Check(psg_store_handle_stretch(state->store, flags, c.stretch, dvals.data(), dout.data(), n, s),
                      "psg_store_handle_stretch");
      else
        device::Check(psg_store_handle_slots(state->store, flags, c.slots.data(), dvals.data(), dout.data(), n, s),
                      "psg_store_handle_slots");
      // answered once the kernel has ended: a polled word, not a stream wait
      device::Check(psg_store_sync(state->store, s), "psg_store_sync");
    } else if (n && flags) {
      if (req_meta.push) CHECK_EQ(n, req_data.vals.size());
      SVector<Key> dkeys = detail::ToDeviceAsync(req_data.keys, dev);
      SVector<Value> dvals;
      if (req_meta.push) dvals = detail::ToDeviceAsync(req_data.vals, dev);
      if (req_meta.pull) dout = PullOutput(server, n, dev, &direct);
      {
        stage::Scope t(req_meta.push ? "server.handle.store.push" : "server.handle.store.pull");
        device::Check(psg_store_handle(state->store, flags, dkeys.data(), 0, dvals.data(), dout.data(), n, s),
                      "psg_store_handle");
      }
      // psg_store_handle returns once the request's keys and vals are no longer
      // read and a Pull's reply is in memory (psg.h), so it can be answered
      // now.  Later requests on this thread's stream are ordered behind it.
      if (state->key_cache) Remember(dkeys, on_dev, on_dev ? 0 : detail::KeyListHash(req_data.keys.data(), n), s);
    } else if (req_meta.push) {
      CHECK_EQ(n, req_data.vals.size());
    }
    if (req_meta.pull) {
      res.keys = req_data.keys;
      // written into the worker's output in place (TakeDirectOut): no values
      if (!direct) res.vals = on_dev ? dout : detail::ToHost(dout);
    }
    server->Response(req_meta, res);
  }

  /* A run of requests queued one behind the other (KVServer::OnReceive), with
   * the result of handling them one at a time in that order (KVApp.h:446-454
   * per request).  Full key lists go to psg_store_run, which reads and writes
   * the store once for the whole run when the lists are one list (Pushes) or
   * interleave (distinct phases of one period of the store: the reference
   * benchmark's layout), and serves them request by request otherwise.  With
   * the key cache, a run of Pushes naming one cached list by its hash is one
   * pass over the cached slots or stretch (psg_store_push_slots_frames).
   * Every request is answered after the run is served. */
  void Run(std::vector<KVRunItem<Value>>& run, KVServer<Value>* server) {
    bool all_push = true, hashed = false;
    for (const auto& it : run) {
      all_push = all_push && it.meta.push && !it.meta.pull;
      hashed = hashed || it.data.keys.size() == 1;
    }
    if (all_push) {
      std::vector<KVMeta> metas;
      std::vector<KVPairs<Value>> datas;
      std::vector<char> spec;
      for (const auto& it : run) {
        metas.push_back(it.meta);
        datas.push_back(it.data);
        spec.push_back(it.spec ? 1 : 0);
      }
      PushRun(metas, datas, server, spec);
      return;
    }
    if (state->key_cache && hashed) {
      // a one-key request names a cached list (LRServer.h:129-135): on its own
      for (const auto& it : run) server->ServeOne(it);
      return;
    }
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerDefaultHandle: the value store lives in HBM and this node has no GPU";
    constexpr int dt = device::DType<Value>();
    CHECK_GE(dt, 0) << "KVServerDefaultHandle: value type not supported by the HBM store";
    if (!state->store)
      device::Check(psg_store_create(PSG_STORE_SORTED, dt, 0, kMaxKey, 0, &state->store), "psg_store_create");
    psg_stream s = device::ThreadStream();
    const size_t k = run.size();
    std::vector<int> ops(k);
    std::vector<uint64_t> ns(k);
    std::vector<SVector<Key>> dkeys(k);
    std::vector<SVector<Value>> dvals(k), douts(k);
    std::vector<const uint64_t*> kp(k);
    std::vector<const void*> vp(k, nullptr);
    std::vector<void*> op(k, nullptr);
    std::vector<char> direct(k, 0);
    for (size_t j = 0; j < k; ++j) {
      const auto& it = run[j];
      const size_t n = it.data.keys.size();
      ops[j] = (it.meta.push ? PSG_PUSH : 0) | (it.meta.pull ? PSG_PULL : 0);
      ns[j] = n;
      if (it.meta.push) CHECK_EQ(n, it.data.vals.size());  // one value per key (KVApp.h:441)
      dkeys[j] = detail::ToDeviceAsync(it.data.keys, dev);
      kp[j] = dkeys[j].data();
      if (it.meta.push) {
        dvals[j] = detail::ToDeviceAsync(it.data.vals, dev);
        vp[j] = dvals[j].data();
      }
      if (it.meta.pull) {
        direct[j] = it.out.size() == n && it.out.on_device();
        douts[j] = direct[j] ? it.out : SVector<Value>::OnDevice(n, dev);
        op[j] = douts[j].data();
      }
    }
    std::vector<int> status(k, PSG_OK);
    bool any_spec = false;
    for (const auto& it : run) any_spec = any_spec || it.spec;
    {
      stage::Scope t("server.handle.store.run");
      ServeRun(any_spec, (int)k, ops.data(), kp.data(), ns.data(), vp.data(), op.data(), s, status.data(),
               [&](int j) { return run[j].spec; });
    }
    // a request refused for a key outside this shard: fatal, as a CHECK,
    // unless its slice was the worker's unconfirmed hint
    for (size_t j = 0; j < k; ++j)
      if (status[j] != PSG_OK && !run[j].spec) device::Check(status[j], "psg_store_run");
    if (state->key_cache)
      for (size_t j = 0; j < k; ++j)
        if (status[j] == PSG_OK)
          Remember(dkeys[j], run[j].data.keys.on_device(),
                   run[j].data.keys.on_device() ? 0 : detail::KeyListHash(run[j].data.keys.data(), ns[j]), s);
    for (size_t j = 0; j < k; ++j) {
      if (status[j] != PSG_OK) {
        server->RunRefuse(run[j].meta);
        continue;
      }
      KVPairs<Value> res;
      if (run[j].meta.pull) {
        res.keys = run[j].data.keys;
        if (!direct[j]) res.vals = run[j].data.keys.on_device() ? douts[j] : detail::ToHost(douts[j]);
      }
      server->RunResponse(run[j].meta, res, direct[j] != 0);
    }
  }

  /* A run of Pushes of one shape (Run). */
  void PushRun(const std::vector<KVMeta>& metas, const std::vector<KVPairs<Value>>& datas, KVServer<Value>* server,
               const std::vector<char>& spec = {}) {
    std::vector<int> status(datas.size(), PSG_OK);
    const int dev = PostOffice::Get()->device();
    CHECK_GE(dev, 0) << "KVServerDefaultHandle: the value store lives in HBM and this node has no GPU";
    constexpr int dt = device::DType<Value>();
    CHECK_GE(dt, 0) << "KVServerDefaultHandle: value type not supported by the HBM store";
    if (!state->store)
      device::Check(psg_store_create(PSG_STORE_SORTED, dt, 0, kMaxKey, 0, &state->store), "psg_store_create");
    psg_stream s = device::ThreadStream();
    const size_t k = datas.size();
    const size_t n = datas[0].keys.size();
    for (const auto& d : datas) {
      CHECK_EQ(d.keys.size(), n);
      if (!(state->key_cache && n == 1)) CHECK_EQ(n, d.vals.size());  // one value per key (KVApp.h:441)
    }
    std::vector<SVector<Value>> dvals(k);
    std::vector<const void*> vp(k);
    if (state->key_cache && n == 1) {
      // cached lists named by their hashes (LRServer.h:129-135); consecutive
      // requests naming one list are one pass
      std::vector<Key> h(k);
      for (size_t j = 0; j < k; ++j) {
        if (datas[j].keys.on_device()) device::CopySync(&h[j], datas[j].keys.data(), sizeof(Key), 1);
        else h[j] = datas[j].keys[0];
      }
      for (size_t i = 0; i < k;) {
        size_t e = i + 1;
        while (e < k && h[e] == h[i]) ++e;
        auto it = state->cache.find(h[i]);
        CHECK(it != state->cache.end()) << "Keys don't exist with hash value: " << h[i];
        Cached& c = it->second;
        Refresh(c, s);
        for (size_t j = i; j < e; ++j) {
          CHECK_EQ(c.keys.size(), datas[j].vals.size());
          dvals[j] = detail::ToDeviceAsync(datas[j].vals, dev);
          vp[j] = dvals[j].data();
        }
        const bool stretch = c.stretch != UINT64_MAX;
        device::Check(psg_store_push_slots_frames(state->store, stretch ? nullptr : c.slots.data(),
                                                  stretch ? c.stretch : 0, vp.data() + i, (int)(e - i),
                                                  c.keys.size(), s),
                      "psg_store_push_slots_frames");
        i = e;
      }
      device::Check(psg_store_sync(state->store, s), "psg_store_sync");
    } else {
      std::vector<SVector<Key>> dkeys(k);
      std::vector<const uint64_t*> kp(k);
      for (size_t j = 0; j < k; ++j) {
        dkeys[j] = detail::ToDeviceAsync(datas[j].keys, dev);
        dvals[j] = detail::ToDeviceAsync(datas[j].vals, dev);
        kp[j] = dkeys[j].data();
        vp[j] = dvals[j].data();
      }
      std::vector<int> ops(k, PSG_PUSH);
      std::vector<uint64_t> ns(k, n);
      bool any_spec = false;
      for (char c : spec) any_spec = any_spec || c;
      ServeRun(any_spec, (int)k, ops.data(), kp.data(), ns.data(), vp.data(), nullptr, s, status.data(),
               [&](int j) { return j < (int)spec.size() && spec[j] != 0; });
      for (size_t j = 0; j < k; ++j)
        if (status[j] != PSG_OK && !(j < spec.size() && spec[j])) device::Check(status[j], "psg_store_run");
      if (state->key_cache)
        for (size_t j = 0; j < k; ++j)
          if (status[j] == PSG_OK)
            Remember(dkeys[j], datas[j].keys.on_device(),
                     datas[j].keys.on_device() ? 0 : detail::KeyListHash(datas[j].keys.data(), n), s);
    }
    for (size_t j = 0; j < metas.size(); ++j) {
      if (status[j] != PSG_OK) server->RunRefuse(metas[j]);
      else server->Response(metas[j], KVPairs<Value>());
    }
  }

  /* A run through psg_store_run_status.  A run holding unconfirmed slices
   * (KVRunItem::spec) is served against this server's own key range, so a
   * slice with a key outside it is refused (nothing of it applied); a request
   * of the run that is not such a slice and was refused only for that
   * narrower range is then served again on the whole range. */
  template <typename IsSpec>
  void ServeRun(bool any_spec, int k, const int* ops, const uint64_t* const* kp, const uint64_t* ns,
                const void* const* vp, void* const* op, psg_stream s, int* status, IsSpec is_spec) {
    int served = 0;
    if (!any_spec) {
      const int rc = psg_store_run_status(state->store, k, ops, kp, ns, vp, op, s, &served, status);
      if (rc != PSG_OK) device::Check(rc, "psg_store_run");
      return;
    }
    const auto& r = PostOffice::Get()->GetServerRanges()[PostOffice::IDToRank(PostOffice::Get()->my_id())];
    device::Check(psg_store_set_key_range(state->store, r.begin, r.end), "psg_store_set_key_range");
    const int rc = psg_store_run_status(state->store, k, ops, kp, ns, vp, op, s, &served, status);
    device::Check(psg_store_set_key_range(state->store, 0, kMaxKey), "psg_store_set_key_range");
    if (rc != PSG_OK) device::Check(rc, "psg_store_run");
    for (int j = 0; j < k; ++j) {
      if (status[j] != PSG_ERR_RANGE || is_spec(j)) continue;
      const int rc1 = psg_store_run_status(state->store, 1, ops + j, kp + j, ns + j, vp + j, op ? op + j : nullptr, s,
                                           &served, status + j);
      if (rc1 != PSG_OK) device::Check(rc1, "psg_store_run");
    }
  }

  psg_store* store() const { return state->store; }
  size_t cached_key_lists() const { return state->cache.size(); }
  /* (key, value) pairs in key order, copied to host */
  void Dump(std::vector<Key>* keys, std::vector<Value>* vals) const {
    keys->clear();
    vals->clear();
    if (!state->store) return;
    psg_store_info info;
    device::Check(psg_store_get_info(state->store, &info), "psg_store_get_info");
    keys->resize(info.size);
    vals->resize(info.size);
    device::Check(psg_store_dump(state->store, keys->data(), vals->data()), "psg_store_dump");
  }

 private:
  uint64_t StoreSize() const {
    psg_store_info info;
    device::Check(psg_store_get_info(state->store, &info), "psg_store_get_info");
    return info.size;
  }
  // cache a full list under its hash (LRServer.h:136-141: the first one wins)
  // a Pull's output: the worker's own slice when it offered one of n values
  // (written in place: no reply frame, no merge), else a fresh HBM array
  static SVector<Value> PullOutput(KVServer<Value>* server, size_t n, int dev, bool* direct) {
    SVector<Value> d = server->TakeDirectOut(n);
    *direct = !d.empty();
    return *direct ? d : SVector<Value>::OnDevice(n, dev);
  }

  // worker_frame: dkeys is the request's own HBM frame (the worker's buffer,
  // or its hipIpc mapping), which the worker may rewrite once the request is
  // answered (psg.h) — the cache keeps a server-owned copy, as the reference
  // keeps its received copy (LRServer.h:139), so a later re-resolve never
  // reads another list, and no worker frame stays mapped.
  void Remember(const SVector<Key>& dkeys, bool worker_frame, uint64_t host_hash, psg_stream s) {
    const size_t n = dkeys.size();
    uint64_t h = host_hash;
    if (dkeys.on_device() && host_hash == 0)
      device::Check(psg_key_list_hash(dkeys.data(), n, &h, s), "psg_key_list_hash");
    if (state->cache.count(h)) return;
    Cached c;
    const int dev = PostOffice::Get()->device();
    if (worker_frame) {
      c.keys = SVector<Key>::OnDevice(n, dev);
      device::Check(psg_memcpy(c.keys.data(), dkeys.data(), n * sizeof(Key), 2 /* D2D */, s), "psg_memcpy D2D");
    } else {
      c.keys = dkeys;  // already the server's copy (ToDeviceAsync of a host frame)
    }
    c.slots = SVector<uint32_t>::OnDevice(n, dev);
    device::Check(psg_store_resolve(state->store, c.keys.data(), n, 0, c.slots.data(), s), "psg_store_resolve");
    device::Check(psg_store_slots_stretch(state->store, c.slots.data(), n, &c.stretch, s), "psg_store_slots_stretch");
    c.store_size = StoreSize();
    state->cache.emplace(h, std::move(c));
  }
  void Refresh(Cached& c, psg_stream s) {
    const uint64_t size = StoreSize();
    if (size == c.store_size) return;
    device::Check(psg_store_resolve(state->store, c.keys.data(), c.keys.size(), 0, c.slots.data(), s),
                  "psg_store_resolve");
    device::Check(psg_store_slots_stretch(state->store, c.slots.data(), c.keys.size(), &c.stretch, s),
                  "psg_store_slots_stretch");
    c.store_size = size;
  }
};

// ============================================================================
// KVServer

template <typename Value>
void KVServer<Value>::OnReceive(const Message& msg) {
  if (msg.meta.simple_app) {
    SimpleApp::OnReceive(msg);
    return;
  }
  const KVMeta meta = MetaOf(msg);
  const uint64_t ordinal = Take(meta.sender);
  bool device_frames, installed;
  RunHandle run;
  {
    std::unique_lock<std::mutex> lk(handle_mu_);
    handle_cv_.wait_for(lk, std::chrono::seconds(30), [this] { return static_cast<bool>(request_handle_); });
    installed = static_cast<bool>(request_handle_);
    device_frames = device_frames_;
    run = run_handle_;
  }
  CHECK(installed) << "no request handle installed 30 s after the first request";
  stage::Scope t_recv(meta.push ? "server.request.push" : "server.request.pull");
  KVPairs<Value> data;
  size_t n = msg.data.size();
  direct_out_ = SVector<Value>();
  direct_taken_ = false;
  if (msg.meta.weighted) {
    // a weighted pooled request: the weights ride behind the offsets
    CHECK(msg.meta.bags) << "a weights frame belongs to a pooled request";
    CHECK_GE(n, (size_t)4) << "a weighted pooled request carries keys, a values frame, its offsets and its weights";
    data.weights = msg.data[--n];
  }
  if (msg.meta.bags) {
    // a pooled request: the bag offsets ride behind the frames every other
    // request carries, which are parsed below as they always were
    CHECK_GE(n, (size_t)3) << "a pooled request carries keys, a values frame and its offsets";
    CHECK(device_frames) << "a pooled request reached a handle that does not take HBM frames";
    data.offsets = msg.data[--n];
  }
  if (n && msg.meta.direct_reply && meta.pull) {
    // the last frame is not request data: it is where this Pull's (or
    // PushPull's) values may go — [keys, out] or [keys, vals, out]
    CHECK_EQ(n, meta.push ? (size_t)3 : (size_t)2);
    data.keys = msg.data[0];
    if (meta.push) data.vals = msg.data[1];
    if (device_frames) {
      direct_out_ = msg.data[n - 1];
      direct_ts_ = meta.timestamp;
      direct_sender_ = meta.sender;
    } else {
      data.keys = detail::ToHost(data.keys);
      data.vals = detail::ToHost(data.vals);
    }
  } else if (n) {
    CHECK_GE(n, (size_t)2);
    data.keys = msg.data[0];
    data.vals = msg.data[1];
    if (n > 2) {
      CHECK_EQ(n, (size_t)3);
      data.lens = msg.data[2];
      CHECK_EQ(data.lens.size(), data.keys.size());
    }
    if (!device_frames) {
      data.keys = detail::ToHost(data.keys);
      data.vals = detail::ToHost(data.vals);
      data.lens = detail::ToHost(data.lens);
    }
  }
  // A run of queued requests.  The reference's receive thread handles the
  // queued messages one at a time, in queue order (Customer.cpp:52-70); a
  // plain request taken here (no lens) may bring along the requests queued
  // right behind it — the very messages the thread would handle next, so
  // nothing is reordered — and the run's handle (KVServerDefaultHandle::Run)
  // serves them as that sequence:
  //   Pushes of one shape (one pass when their lists are one list: nw workers
  //     of a BSP round, or a worker's Pushes in flight), and
  //   requests of distinct senders, Pushes and Pulls (one pass when their
  //     lists interleave: the reference benchmark's `kMaxKey / num * i + rank`
  //     at nw workers, tests/test_kv_app_benchmark.cpp:47-52);
  // request by request otherwise.
  if (run && device_frames && detail::PushRunsOn() && PlainRequest(msg)) {
    const size_t kbytes = msg.data[0].size(), vbytes = msg.data[1].size();
    auto push_shape = [&](const Message& m) {
      return m.meta.push && !m.meta.pull && !m.meta.direct_reply && m.data.size() == 2 && m.data[0].size() == kbytes &&
             m.data[1].size() == vbytes;
    };
    bool all_push = push_shape(msg), distinct = true;
    std::vector<KVRunItem<Value>> items(1);
    items[0].meta = meta;
    items[0].data = data;
    items[0].out = direct_out_;
    items[0].spec = msg.meta.spec_slice;
    auto mate = [&](const Message& m) {
      if (m.meta.app_id != msg.meta.app_id || !PlainRequest(m)) return false;
      if (all_push && push_shape(m)) return true;
      if (!distinct || !detail::MixedRunsOn()) return false;
      for (const auto& it : items)
        if (it.meta.sender == m.meta.sender) return false;
      return true;
    };
    // The gather window (PS_RUN_GATHER_US, default 120; 0: off): when fewer
    // requests are queued than the senders this server has heard from lately,
    // wait up to that long for theirs to arrive — the requests of one step
    // reach a server microseconds apart, and a request taken alone costs a
    // whole pass over the store's lines.  The wait ends as soon as the head of
    // the queue is a message that may not join (PopIf's refusal: a message
    // that arrives while the window checks its senders is still taken).
    // A window that keeps timing out with nothing gained (a sender stopped
    // sending) is skipped for the next 64 requests.
    // With the ordinal rule (detail::RunGatherOrdinal) the window waits only
    // for the senders behind the run, for up to PS_RUN_GATHER_ORD_US.
    const bool by_ordinal = detail::RunGatherOrdinal() && detail::RunGatherMicros() > 0;
    int gather_us = gather_cool_ > 0 ? 0 : by_ordinal ? detail::RunGatherOrdMicros() : detail::RunGatherMicros();
    if (gather_us > 0 && !by_ordinal && detail::RunGatherAutoCap() > 0)
      gather_us = std::min(detail::RunGatherAutoCap(), std::max(gather_us, (int)run_us_));
    if (gather_cool_ > 0) --gather_cool_;
    const size_t want = gather_us > 0 ? RecentSenders(meta.sender) : 0;
    uint64_t low = ordinal;  // the run's lowest ordinal
    const auto t_gather = std::chrono::steady_clock::now();
    bool waited = false;
    Message next;
    int why = 0;
    while ((int)items.size() < kMaxRun) {
      bool refused = false;
      if (!customer_->TakeQueued(mate, &next, &refused)) {
        // (the head of the queue may not join: the run ends here, in queue order)
        if (refused) {
          why = 2;
          break;
        }
        const bool more = gather_us > 0 && (by_ordinal ? SendersBehind(items, low) : items.size() < want);
        if (!more) {
          why = 1;
          break;
        }
        if (std::chrono::steady_clock::now() - t_gather > std::chrono::microseconds(gather_us)) {
          if (by_ordinal) (void)SendersBehind(items, low, true);
          if (!waited && ++gather_idle_ >= 4) {
            gather_idle_ = 0;
            gather_cool_ = 64;
          }
          why = 3;
          break;
        }
        __builtin_ia32_pause();
        continue;
      }
      if (items.size() >= 1 && std::chrono::steady_clock::now() - t_gather > std::chrono::microseconds(1)) {
        waited = true;  // a request joined after the wait began
        gather_idle_ = 0;
      }
      NoteSender(next.meta.sender);
      low = std::min(low, Take(next.meta.sender));
      KVRunItem<Value> it;
      it.meta = MetaOf(next);
      for (const auto& o : items) distinct = distinct && o.meta.sender != it.meta.sender;
      all_push = all_push && push_shape(next);
      it.data.keys = next.data[0];
      if (next.meta.push) it.data.vals = next.data[1];
      if (next.meta.direct_reply) it.out = next.data[next.data.size() - 1];
      it.spec = next.meta.spec_slice;
      items.push_back(std::move(it));
    }
    // (a plain request on its own goes to the run handle too: the store
    // serves it as a strided pass when it knows its list's place in a learnt
    // interleaved layout, else as one request)
    detail::TraceGather(PostOffice::Get()->my_id(), meta.sender, ordinal, items.size(), why,
                        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_gather).count());
    if (items.size() > 1 || detail::MixedRunsOn()) {
      direct_out_ = SVector<Value>();
      for (size_t j = 0; j < items.size(); ++j)
        detail::TraceRequest(PostOffice::Get()->my_id(), items[j].meta, items[j].data.keys.size(), items.size(), j);
      const auto t_run = std::chrono::steady_clock::now();
      run(items, this);
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_run).count();
      run_us_ = run_us_ > 0 ? 0.75 * run_us_ + 0.25 * us : us;
      return;
    }
  }
  CHECK(!msg.meta.spec_slice) << "an unconfirmed slice reached a handle that does not check it";
  detail::TraceRequest(PostOffice::Get()->my_id(), meta, data.keys.size(), 1, 0);
  // called in place: a handle keeps its state across requests (KVApp.h:457)
  {
    stage::Scope t("server.handle");
    request_handle_(meta, data, this);
  }
  direct_out_ = SVector<Value>();
  direct_taken_ = false;
}

template <typename Value>
void KVServer<Value>::Response(const KVMeta& req, const KVPairs<Value>& res) {
  // the handle wrote this Pull's values into the worker's output in place
  Reply(req, res,
        direct_taken_.load() && req.timestamp == direct_ts_.load() && req.sender == direct_sender_.load());
}

template <typename Value>
void KVServer<Value>::Reply(const KVMeta& req, const KVPairs<Value>& res, bool direct, bool refused) {
  stage::Scope t("server.response", res.keys.size() * sizeof(Key) + res.vals.size() * sizeof(Value));
  Message msg;
  msg.meta.app_id = customer_->app_id();
  msg.meta.customer_id = req.customer_id;
  msg.meta.request = false;
  msg.meta.push = req.push;
  msg.meta.pull = req.pull;
  msg.meta.head = req.cmd;
  msg.meta.timestamp = req.timestamp;
  msg.meta.receiver = req.sender;
  // tells the worker that HBM frames reach this handle without a copy back
  msg.meta.hbm_handle = device_frames_.load();
  msg.meta.direct_reply = direct;
  if (msg.meta.direct_reply) CHECK(res.vals.empty()) << "a direct reply carries no values";
  // tells the worker it may send this server unconfirmed slices (KVWorker::Send)
  msg.meta.spec_slice = TakesSpecSlices();
  msg.meta.refused = refused;
  if (refused) CHECK(res.keys.empty() && !direct) << "a refusal carries nothing";
  if (res.keys.size()) {
    msg.AddData(res.keys);
    msg.AddData(res.vals);
    if (res.lens.size()) msg.AddData(res.lens);
  }
  PostOffice::Get()->van()->Send(msg);
}

// ============================================================================
// KVWorker

template <typename Value>
void KVWorker<Value>::DefaultSlicer(Data& send, const std::vector<Range>& ranges, SlicedKVs* sliced) {
  const size_t n = ranges.size();
  sliced->resize(n);
  std::vector<uint64_t> pos(n + 1, 0), vpos(n + 1, 0);
  const size_t nkeys = send.keys.size();
  if (send.keys.on_device() && n == 1 && send.lens.empty()) {
    // one server owns [0, kMaxKey): the slice is the whole request, no kernel
    // and no host sync.  The one key the reference's slicer would reject
    // (kMaxKey itself, KVApp.h:544) is rejected by the server's range check.
    CHECK_EQ(nkeys ? send.vals.size() / nkeys * nkeys : send.vals.size(), send.vals.size());
    pos[1] = nkeys;
    vpos[1] = send.vals.size();
  } else if (send.keys.on_device()) {
    stage::Scope t("worker.slice.device", nkeys * sizeof(Key));
    if (send.lens.size()) {
      CHECK_EQ(send.keys.size(), send.lens.size());
      CHECK(send.lens.on_device()) << "device keys need device lens";
    }
    device::SliceKeys(send.keys.data(), nkeys, send.lens.size() ? send.lens.data() : nullptr,
                      send.vals.size(), ranges, &pos, &vpos);
  } else {
    const Key* begin = send.keys.begin();
    const Key* end = send.keys.end();
    for (size_t i = 0; i < n; ++i) {
      if (i == 0) {
        pos[0] = std::lower_bound(begin, end, ranges[0].begin) - begin;
        begin += pos[0];
      } else {
        CHECK_EQ(ranges[i - 1].end, ranges[i].begin);
      }
      size_t len = std::lower_bound(begin, end, ranges[i].end) - begin;
      begin += len;
      pos[i + 1] = pos[i] + len;
    }
    CHECK_EQ(pos[n], nkeys);
    if (nkeys) {
      if (send.lens.empty()) {
        const size_t k = send.vals.size() / nkeys;
        CHECK_EQ(k * nkeys, send.vals.size());
        for (size_t i = 0; i <= n; ++i) vpos[i] = pos[i] * k;
      } else {
        CHECK_EQ(nkeys, send.lens.size());
        SVector<int> hl = detail::ToHost(send.lens);
        uint64_t acc = 0;
        for (size_t i = 0; i < n; ++i) {
          vpos[i] = acc;
          for (size_t j = pos[i]; j < pos[i + 1]; ++j) acc += hl[j];
        }
        vpos[n] = acc;
      }
    }
  }
  for (size_t i = 0; i < n; ++i) {
    auto& s = sliced->at(i);
    s.first = pos[i + 1] != pos[i];
    if (!s.first) continue;
    s.second.keys = send.keys.Slice(pos[i], pos[i + 1]);
    s.second.vals = send.vals.Slice(vpos[i], vpos[i + 1]);
    if (send.lens.size()) s.second.lens = send.lens.Slice(pos[i], pos[i + 1]);
  }
}

template <typename Value>
void KVWorker<Value>::Send(int timestamp, bool push, bool pull, int cmd, const Data& kvs, bool direct,
                           const SVector<Value>* outs) {
  stage::Scope t_send(push ? "worker.send.push" : "worker.send.pull");
  SlicedKVs sliced;
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  const size_t ns = ranges.size();
  // Unconfirmed slices (PS_SPEC_SLICE=0: off): an HBM key list this thread sliced
  // before is sent on the bounds it had then, without the slicer's kernel and
  // readback, when every server's handle checks each key against its own
  // range (a wrong bound puts some key outside its server's range; that
  // server refuses its slice, applying nothing, and Refused re-sends those
  // keys sliced for real).  Not with lens, a custom slicer, or a Pull merged
  // on the host (its replies must be the servers' slices).
  bool spec = false;
  std::vector<uint64_t> hint;
  const size_t nkeys = kvs.keys.size();
  if (detail::SpecSliceOn() && default_slicer_ && ns > 1 && nkeys && kvs.keys.on_device() && kvs.lens.empty() &&
      (!pull || direct) && servers_take_spec_.load()) {
    bool stale = false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      stale = spec_stale_.erase(kvs.keys.data()) > 0;
    }
    int found = 0;
    hint.assign(ns + 1, 0);
    if (!stale)
      device::Check(psg_slice_hint(kvs.keys.data(), nkeys, (int)ns, ranges[0].begin, hint.data(), &found),
                    "psg_slice_hint");
    if (found && hint[ns] == nkeys) {
      const size_t per = kvs.vals.size() / nkeys;
      CHECK_EQ(per * nkeys, kvs.vals.size());
      sliced.resize(ns);
      for (size_t i = 0; i < ns; ++i) {
        auto& sl = sliced[i];
        sl.first = hint[i + 1] != hint[i];
        if (!sl.first) continue;
        sl.second.keys = kvs.keys.Slice(hint[i], hint[i + 1]);
        sl.second.vals = kvs.vals.Slice(hint[i] * per, hint[i + 1] * per);
      }
      spec = true;
      SpecSend sp;
      sp.push = push;
      sp.pull = pull;
      sp.direct = direct;
      sp.cmd = cmd;
      sp.kvs = kvs;
      sp.has_outs = outs != nullptr;
      if (outs) sp.outs = *outs;
      sp.pos = hint;
      std::lock_guard<std::mutex> lk(mu_);
      spec_sends_[timestamp] = std::move(sp);
    }
  }
  if (!spec) slicer_(const_cast<Data&>(kvs), ranges, &sliced);
  SendSliced(timestamp, push, pull, cmd, kvs, sliced, direct, outs, spec);
}

template <typename Value>
void KVWorker<Value>::SendSliced(int timestamp, bool push, bool pull, int cmd, const Data& kvs, SlicedKVs& sliced,
                                 bool direct, const SVector<Value>* outs, bool spec) {
  int skipped = 0;
  for (auto& sl : sliced)
    if (!sl.first) ++skipped;
  customer_->AddResponse(timestamp, skipped);
  if ((size_t)skipped == sliced.size()) RunCallback(timestamp);
  for (size_t i = 0; i < sliced.size(); ++i) {
    if (!sliced[i].first) continue;
    SendOne(timestamp, push, pull, cmd, kvs.priority, kvs, sliced[i].second, direct, outs, (int)i, spec);
  }
}

template <typename Value>
void KVWorker<Value>::SendBounds(int timestamp, bool push, bool pull, int cmd, const Data& kvs,
                                 const std::vector<uint64_t>& pos, bool direct, const SVector<Value>* outs) {
  stage::Scope t_send(push ? "worker.send.push" : "worker.send.pull");
  CHECK_GE(pos.size(), (size_t)2);
  const size_t ns = pos.size() - 1;
  const size_t nkeys = kvs.keys.size();
  CHECK_EQ(pos[ns], nkeys);
  const size_t per = nkeys ? kvs.vals.size() / nkeys : 0;
  CHECK_EQ(per * nkeys, kvs.vals.size());
  SlicedKVs sliced(ns);
  for (size_t i = 0; i < ns; ++i) {
    auto& sl = sliced[i];
    sl.first = pos[i + 1] != pos[i];
    if (!sl.first) continue;
    sl.second.keys = kvs.keys.Slice(pos[i], pos[i + 1]);
    sl.second.vals = kvs.vals.Slice(pos[i] * per, pos[i + 1] * per);
  }
  SendSliced(timestamp, push, pull, cmd, kvs, sliced, direct, outs, false);
}

// The Z forms of the any-order calls (see the class comment).  The frames of a
// routed request — routed keys, perm, gathered values, the routed output — are
// held by the completion's captures until it has run.
template <typename Value>
int KVWorker<Value>::SendAny(const SVector<Key>& keys, const SVector<Value>* vals, SVector<Value>* outs, int cmd,
                             const Callback& cb, int priority) {
  const bool push = vals != nullptr, pull = outs != nullptr;
  CHECK(default_slicer_) << "an Any call routes by the servers' key ranges: it cannot be combined with a custom slicer";
  CHECK(keys.empty() || keys.on_device()) << "the Z forms of the Any calls take keys in HBM (host keys: PushAny / "
                                             "PullAny / PushPullAny)";
  const size_t n = keys.size();
  if (push) CHECK_EQ(n ? vals->size() / n * n : vals->size(), vals->size()) << "vals hold a whole number of rows";
  if (pull) CHECK_EQ(n ? outs->size() / n * n : outs->size(), outs->size()) << "the output holds a whole number of rows";
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  const size_t ns = ranges.size();
  if (ns == 1 || n == 0) {  // the list goes on whole
    if (push && pull) return ZPushPull(keys, *vals, outs, nullptr, cmd, cb, priority);
    return push ? ZPush(keys, *vals, {}, cmd, cb, priority) : ZPull(keys, outs, nullptr, cmd, cb, priority);
  }
  // (a Push without values — the row handles' kRowErase — carries only keys)
  if (push && vals->size()) CHECK(vals->on_device()) << "HBM keys need HBM values";
  if (pull) CHECK(outs->on_device() && outs->size()) << "HBM keys need a sized HBM output";
  const int dev = keys.device();
  psg_stream st = device::ThreadStream();
  std::vector<uint64_t> begins(ns), ends(ns), pos(ns + 1, 0);
  for (size_t i = 0; i < ns; ++i) begins[i] = ranges[i].begin, ends[i] = ranges[i].end;
  SVector<Key> rkeys = SVector<Key>::OnDevice(n, dev);
  SVector<uint32_t> perm = SVector<uint32_t>::OnDevice(n, dev);
  int identity = 0;
  {
    stage::Scope t("worker.route.device", n * sizeof(Key));
    device::Check(psg_route(keys.data(), n, (int)ns, begins.data(), ends.data(), rkeys.data(), perm.data(), pos.data(),
                            &identity, st),
                  "psg_route");
  }
  Data kvs;
  kvs.priority = priority;
  const bool direct = pull && detail::DirectReplyOn();
  if (identity) {
    // already partitioned: the caller's own arrays on the route's bounds
    kvs.keys = keys;
    if (push) kvs.vals = *vals;
    if (pull && !push && direct) kvs.vals = *outs;
    const int ts = pull ? AddPullCB(keys, outs, (SVector<int>*)nullptr, cmd, cb, true) : customer_->NewRequest(kServerGroup);
    if (!pull) AddCallback(ts, cb);
    SendBounds(ts, push, pull, cmd, kvs, pos, direct, push && pull && direct ? outs : nullptr);
    return ts;
  }
  kvs.keys = rkeys;
  SVector<Value> rvals;
  if (push && vals->size()) {  // no values: nothing to gather (psg_rows_gather refuses rows of 0 bytes)
    const size_t row = vals->size() / n * sizeof(Value);
    rvals = SVector<Value>::OnDevice(vals->size(), dev);
    stage::Scope t("worker.route.gather", 2 * vals->size() * sizeof(Value));
    device::Check(psg_rows_gather(rvals.data(), vals->data(), perm.data(), n, row, st), "psg_rows_gather");
    kvs.vals = rvals;
  }
  // the servers read the frames on streams of their own
  device::Check(psg_stream_sync(st), "psg_stream_sync");
  if (!pull) {
    const int ts = customer_->NewRequest(kServerGroup);
    AddCallback(ts, [rkeys, perm, rvals, cb]() {
      if (cb) cb();
    });
    SendBounds(ts, true, false, cmd, kvs, pos, false, nullptr);
    return ts;
  }
  auto routs = std::make_shared<SVector<Value>>(SVector<Value>::OnDevice(outs->size(), dev));
  if (!push && direct) kvs.vals = *routs;
  const SVector<Value> out = *outs;  // shares the caller's buffer
  const int ts = AddPullCB(rkeys, routs.get(), (SVector<int>*)nullptr, cmd,
                           [rkeys, perm, rvals, routs, out, n, cb]() mutable {
                             const size_t row = out.size() / n * sizeof(Value);
                             psg_stream s = device::ThreadStream();
                             {
                               stage::Scope t("worker.route.scatter", 2 * out.size() * sizeof(Value));
                               device::Check(psg_rows_scatter(out.data(), routs->data(), perm.data(), n, row, s),
                                             "psg_rows_scatter");
                               device::Check(psg_stream_sync(s), "psg_stream_sync");
                             }
                             routs.reset();
                             rkeys = SVector<Key>();
                             perm = SVector<uint32_t>();
                             rvals = SVector<Value>();
                             if (cb) cb();
                           },
                           true);
  SendBounds(ts, push, true, cmd, kvs, pos, direct, push && direct ? routs.get() : nullptr);
  return ts;
}

// The pooled calls (see the class comment).  The request's frames — routed keys,
// perm, the servers' offsets and, for a Pull, one partial frame per server that
// owns ids — are held by the completion's captures until it has run.
template <typename Value>
int KVWorker<Value>::SendPooled(const SVector<Key>& keys, const SVector<uint64_t>& offsets, const SVector<Value>* grads,
                                SVector<Value>* out, bool step, bool all, const Callback& cb, int priority,
                                const SVector<float>* weights, bool mean) {
  const bool pull = out != nullptr;
  const char* who = weights ? (pull ? "ZPullPooledWeighted" : "ZPushPooledWeighted")
                    : mean  ? (pull ? "ZPullPooledMean" : all ? "ZPushPooledMeanAll" : "ZPushPooledMean")
                            : (pull ? "ZPullPooled" : all ? "ZPushPooledAll" : "ZPushPooled");
  CHECK(!(weights && mean)) << "a mean bag takes no weights";
  CHECK(!(pull && all)) << "ZPullPooled asks the servers that own ids";
  CHECK(default_slicer_) << who << " routes by the servers' key ranges: it cannot be combined with a custom slicer";
  CHECK(keys.empty() || keys.on_device()) << who << ": keys live in HBM";
  CHECK(offsets.size() >= 1 && offsets.on_device()) << who << ": offsets are nb + 1 words in HBM";
  constexpr int dt = device::DType<Value>();
  CHECK_GE(dt, 0) << who << ": value type not supported by the HBM table";
  const size_t n = keys.size(), nb = offsets.size() - 1;
  const SVector<Value>& vals = pull ? *out : *grads;
  CHECK(vals.empty() || vals.on_device()) << who << ": " << (pull ? "out" : "grads") << " lives in HBM";
  CHECK_EQ(nb ? vals.size() / nb * nb : (size_t)0, vals.size())
      << who << ": " << (pull ? "out" : "grads") << " holds a whole number of values per bag";
  const size_t count = vals.size();  // nb * k
  if (weights) {
    CHECK_EQ(weights->size(), n) << who << ": one weight per key";
    CHECK(weights->empty() || weights->on_device()) << who << ": weights live in HBM";
  }
  if (!pull && (weights || mean))
    CHECK((std::is_same<Value, float>::value)) << who << ": the table's update takes float gradients only";
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  const size_t ns = ranges.size();
  const int dev = offsets.device();
  psg_stream st = device::ThreadStream();
  // the route, as SendAny's
  std::vector<uint64_t> pos(ns + 1, 0);
  SVector<Key> skeys = keys;  // the keys as sent
  SVector<uint32_t> perm;
  if (ns == 1 || n == 0) {
    pos[ns] = n;
  } else {
    std::vector<uint64_t> begins(ns), ends(ns);
    for (size_t i = 0; i < ns; ++i) begins[i] = ranges[i].begin, ends[i] = ranges[i].end;
    SVector<Key> rkeys = SVector<Key>::OnDevice(n, dev);
    perm = SVector<uint32_t>::OnDevice(n, dev);
    int identity = 0;
    stage::Scope t("worker.route.device", n * sizeof(Key));
    device::Check(psg_route(keys.data(), n, (int)ns, begins.data(), ends.data(), rkeys.data(), perm.data(), pos.data(),
                            &identity, st),
                  "psg_route");
    if (identity) perm = SVector<uint32_t>();  // already partitioned: the caller's own keys
    else skeys = rkeys;
  }
  // the weights as sent: routed like the keys (in memory when psg_route_bags returns)
  SVector<float> sweights;
  if (weights) {
    sweights = *weights;
    if (!perm.empty()) {
      sweights = SVector<float>::OnDevice(n, dev);
      stage::Scope t("worker.route.gather", 2 * n * sizeof(float));
      device::Check(psg_rows_gather(sweights.data(), weights->data(), perm.data(), n, sizeof(float), st),
                    "psg_rows_gather");
    }
  }
  // every server's share of every bag; returns once the offsets frame is in
  // memory (the servers read the frames on streams of their own)
  SVector<uint64_t> so = SVector<uint64_t>::OnDevice(ns * (nb + 1), dev);
  {
    stage::Scope t("worker.route.bags", (ns + 1) * (nb + 1) * sizeof(uint64_t));
    const int rc = psg_route_bags(offsets.data(), nb, perm.empty() ? nullptr : perm.data(), n, (int)ns, pos.data(),
                                  so.data(), st);
    CHECK(rc == PSG_OK) << who << ": " << psg_last_error() << " (nothing was sent)";
  }
  if (nb == 0) device::Check(psg_stream_sync(st), "psg_stream_sync");  // (no kernel ran: the route's writes)
  // a mean Push: the gradient rows divided once, behind the offsets' check; the
  // frame is then a plain pooled Push's
  SVector<Value> scaled;
  if (mean && !pull && count) {
    scaled = SVector<Value>::OnDevice(count, dev);
    if constexpr (std::is_same<Value, float>::value) {
      stage::Scope t("worker.push.scale_mean", 2 * count * sizeof(Value));
      device::Check(psg_pool_scale_mean(scaled.data(), grads->data(), offsets.data(), nb, (uint32_t)(count / nb), st),
                    "psg_pool_scale_mean");
      device::Check(psg_stream_sync(st), "psg_stream_sync");
    }
    grads = &scaled;
  }
  // one server serves a mean Pull whole (the one-table mean); several answer sums
  const bool mean_whole = mean && pull && ns == 1;
  // the servers that are sent to: those that own ids, or (all) every one
  int owners = 0;
  for (size_t s = 0; s < ns; ++s) owners += all || pos[s + 1] != pos[s] ? 1 : 0;
  const bool direct = pull && detail::DirectReplyOn();
  // a Pull's partial frames, by server rank; one server: the output itself
  auto frames = std::make_shared<std::vector<SVector<Value>>>(ns);
  if (pull)
    for (size_t s = 0; s < ns; ++s)
      if (pos[s + 1] != pos[s]) (*frames)[s] = ns == 1 ? *out : SVector<Value>::OnDevice(count, dev);
  const int ts = customer_->NewRequest(kServerGroup);
  if (!pull) {
    AddCallback(ts, [skeys, perm, so, sweights, scaled, cb]() {
      if (cb) cb();
    });
  } else {
    const SVector<Value> result = *out;  // shares the caller's buffer
    // (a mean over several servers reads the caller's offsets: kept alive here)
    AddCallback(ts, [this, ts, skeys, perm, so, sweights, offs = offsets, mean, mean_whole, nb, frames, result, count, owners,
                     cb]() mutable {
      std::vector<Reply> kvs;
      {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = recv_kvs_.find(ts);
        if (it != recv_kvs_.end()) {
          kvs.swap(it->second);
          recv_kvs_.erase(it);
        }
      }
      CHECK_EQ((int)kvs.size(), owners) << "ZPullPooled: lost some servers?";
      psg_stream s = device::ThreadStream();
      stage::Scope t("worker.pull.pool_reduce", (owners + 1) * count * sizeof(Value));
      for (const Reply& r : kvs) {
        const size_t rank = (size_t)PostOffice::IDToRank(r.sender);
        CHECK(rank < frames->size() && !(*frames)[rank].empty()) << "ZPullPooled: a reply from a server that was sent nothing";
        if (r.direct) continue;  // written into the offered frame in place
        CHECK_EQ(r.kv.vals.size(), count) << "ZPullPooled: a server answers one row per bag";
        (*frames)[rank] = detail::ToDevice(r.kv.vals, result.device());
      }
      std::vector<const void*> parts;  // in rank order
      for (const auto& f : *frames)
        if (!f.empty()) parts.push_back(f.data());
      if (owners == 0) {
        device::Check(psg_memset(result.data(), 0, count * sizeof(Value), s), "psg_memset");  // every bag is empty: +0
      } else if (mean && !mean_whole) {
        if (count)
          device::Check(psg_pool_reduce_mean(result.data(), parts.data(), (int)parts.size(), offs.data(), nb,
                                             (uint32_t)(count / nb), device::DType<Value>(), s),
                        "psg_pool_reduce_mean");
      } else if (!(parts.size() == 1 && parts[0] == (const void*)result.data())) {
        if (mean_whole)  // the server's mean as it is (a fold from +0 would lose a -0)
          device::Check(psg_memcpy(result.data(), parts[0], count * sizeof(Value), 2 /* D2D */, s), "psg_memcpy D2D");
        else
          device::Check(psg_pool_reduce(result.data(), parts.data(), (int)parts.size(), count, device::DType<Value>(), s),
                        "psg_pool_reduce");
      }
      device::Check(psg_stream_sync(s), "psg_stream_sync");
      frames.reset();
      skeys = SVector<Key>();
      perm = SVector<uint32_t>();
      so = SVector<uint64_t>();
      sweights = SVector<float>();
      offs = SVector<uint64_t>();
      if (cb) cb();
    });
  }
  stage::Scope t_send(pull ? "worker.send.pull" : "worker.send.push");
  customer_->AddResponse(ts, (int)ns - owners);
  if (owners == 0) RunCallback(ts);
  const int cmd = mean_whole ? kRowLookupPooledMean : pull ? kRowLookupPooled : step ? kRowUpdatePooledStep : kRowUpdatePooled;
  for (size_t s = 0; s < ns; ++s) {
    if (!all && pos[s + 1] == pos[s]) continue;
    Message msg;
    msg.meta.app_id = customer_->app_id();
    msg.meta.customer_id = customer_->customer_id();
    msg.meta.request = true;
    msg.meta.push = !pull;
    msg.meta.pull = pull;
    msg.meta.head = cmd;
    msg.meta.timestamp = ts;
    msg.meta.receiver = PostOffice::ServerRankToID((int)s);
    msg.meta.priority = priority;
    msg.meta.direct_reply = direct;
    msg.meta.bags = true;
    msg.AddData(skeys.Slice(pos[s], pos[s + 1]));
    msg.AddData(pull ? (direct ? (*frames)[s] : SVector<Value>()) : *grads);
    msg.AddData(so.Slice(s * (nb + 1), (s + 1) * (nb + 1)));
    if (weights) {
      msg.meta.weighted = true;
      msg.AddData(sweights.Slice(pos[s], pos[s + 1]));
    }
    PostOffice::Get()->van()->Send(msg);
  }
  return ts;
}

// The host-vector forms: the same definition on the host.
template <typename Value>
int KVWorker<Value>::SendAnyHost(const std::vector<Key>& keys, const std::vector<Value>* vals,
                                 std::vector<Value>* outs, int cmd, const Callback& cb, int priority) {
  const bool push = vals != nullptr, pull = outs != nullptr;
  CHECK(default_slicer_) << "an Any call routes by the servers' key ranges: it cannot be combined with a custom slicer";
  const size_t n = keys.size();
  if (n == 0) {
    if (push && pull) return PushPull(keys, *vals, outs, nullptr, cmd, cb, priority);
    return push ? Push(keys, *vals, {}, cmd, cb, priority) : Pull(keys, outs, nullptr, cmd, cb, priority);
  }
  if (push) CHECK_EQ(vals->size() / n * n, vals->size()) << "vals hold a whole number of rows";
  if (pull) CHECK_EQ(outs->size() / n * n, outs->size()) << "the output holds a whole number of rows";
  CHECK_LE(n, (size_t)0xfffffffeull);
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  const size_t ns = ranges.size();
  for (size_t i = 1; i < ns; ++i) CHECK_EQ(ranges[i - 1].end, ranges[i].begin);
  // a stable counting pass whose digit is the owner
  std::vector<uint32_t> owner(n);
  std::vector<uint64_t> pos(ns + 1, 0);
  bool identity = true;
  for (size_t i = 0; i < n; ++i) {
    const Key k = keys[i];
    CHECK(k >= ranges[0].begin && k < ranges[ns - 1].end) << "key " << k << " lies outside the server ranges";
    size_t o = 0;
    while (k >= ranges[o].end) ++o;
    owner[i] = (uint32_t)o;
    ++pos[o + 1];
    if (i && owner[i] < owner[i - 1]) identity = false;
  }
  for (size_t s = 0; s < ns; ++s) pos[s + 1] += pos[s];
  auto perm = std::make_shared<std::vector<uint32_t>>();
  Data kvs;
  kvs.priority = priority;
  if (identity) {
    kvs.keys = SVector<Key>(keys);
    if (push) kvs.vals = SVector<Value>(*vals);
  } else {
    perm->resize(n);
    std::vector<uint64_t> at(pos.begin(), pos.end() - 1);
    for (size_t i = 0; i < n; ++i) (*perm)[at[owner[i]]++] = (uint32_t)i;
    kvs.keys = SVector<Key>::Uninitialized(n);
    for (size_t r = 0; r < n; ++r) kvs.keys[r] = keys[(*perm)[r]];
    if (push && vals->size()) {  // no values: the routed request carries only keys
      const size_t per = vals->size() / n;
      kvs.vals = SVector<Value>::Uninitialized(vals->size());
      for (size_t r = 0; r < n; ++r)
        std::memcpy(kvs.vals.data() + r * per, vals->data() + (size_t)(*perm)[r] * per, per * sizeof(Value));
    }
  }
  if (!pull) {
    const int ts = customer_->NewRequest(kServerGroup);
    AddCallback(ts, cb);
    SendBounds(ts, true, false, cmd, kvs, pos, false, nullptr);
    return ts;
  }
  auto routs = std::make_shared<SVector<Value>>();
  const int ts = AddPullCB(kvs.keys, routs.get(), (SVector<int>*)nullptr, cmd,
                           [routs, perm, outs, n, identity, cb]() {
                             if (outs->empty())
                               outs->resize(routs->size());
                             else
                               CHECK_EQ(outs->size(), routs->size());
                             const size_t per = routs->size() / n;
                             if (identity) {
                               std::memcpy(outs->data(), routs->data(), routs->size() * sizeof(Value));
                             } else {
                               for (size_t r = 0; r < n; ++r)
                                 std::memcpy(outs->data() + (size_t)(*perm)[r] * per, routs->data() + r * per,
                                             per * sizeof(Value));
                             }
                             if (cb) cb();
                           },
                           true);
  SendBounds(ts, push, true, cmd, kvs, pos, false, nullptr);
  return ts;
}

// One server's slice of a request (Send, SendPieces): `kv` is a slice of
// `whole`, the request as the caller gave it.
template <typename Value>
void KVWorker<Value>::SendOne(int timestamp, bool push, bool pull, int cmd, int priority, const Data& whole,
                              const Data& kv, bool direct, const SVector<Value>* outs, int server_rank, bool spec) {
  Message msg;
  msg.meta.app_id = customer_->app_id();
  msg.meta.customer_id = customer_->customer_id();
  msg.meta.request = true;
  msg.meta.push = push;
  msg.meta.pull = pull;
  msg.meta.head = cmd;
  msg.meta.timestamp = timestamp;
  msg.meta.receiver = PostOffice::ServerRankToID(server_rank);
  msg.meta.priority = priority;
  msg.meta.direct_reply = direct;
  msg.meta.spec_slice = spec;
  SVector<Value> out_slice;
  if (direct && outs) {
    // a PushPull: the output slice at this server's values' offset, found
    // from where its vals slice sits in the request (a slicer that copied
    // the values instead of slicing them gets no offer)
    const Value* base = whole.vals.data();
    const Value* v = kv.vals.data();
    if (kv.vals.size() && v >= base && v + kv.vals.size() <= base + whole.vals.size()) {
      const size_t off = (size_t)(v - base);
      out_slice = outs->Slice(off, off + kv.vals.size());
    } else {
      msg.meta.direct_reply = false;
    }
  }
  bool drop_vals = false;
  if (direct && !outs) {
    // a Pull whose vals frame is the caller's output: offered only when this
    // server's vals slice is the output at its keys' offset (a custom slicer
    // that copied or remapped the values gets no offer, and a plain Pull
    // request without values, as the reference sends)
    const Key* kbase = whole.keys.data();
    const Key* k = kv.keys.data();
    const size_t per = whole.keys.size() ? whole.vals.size() / whole.keys.size() : 0;
    const bool keys_inside = kv.keys.size() && k >= kbase && k + kv.keys.size() <= kbase + whole.keys.size();
    const bool ok = keys_inside && per && kv.vals.size() == kv.keys.size() * per &&
                    kv.vals.data() == whole.vals.data() + (size_t)(k - kbase) * per;
    if (!ok) {
      msg.meta.direct_reply = false;
      drop_vals = true;
    }
  }
  if (kv.keys.size()) {
    msg.AddData(kv.keys);
    msg.AddData(drop_vals ? SVector<Value>() : kv.vals);
    if (kv.lens.size()) msg.AddData(kv.lens);
    if (msg.meta.direct_reply && outs) msg.AddData(out_slice);
  }
  PostOffice::Get()->van()->Send(msg);
}

// A server refused its unconfirmed slice [pos[r], pos[r+1]) of request
// `timestamp` (a key outside its range: the key list changed since it was
// last sliced; nothing of that slice was applied).  The list is sliced for
// real and those keys go to the servers that own them, as requests of the same
// timestamp; the request now waits for their replies too.  The servers that
// took their slices hold exactly their keys (each accepted slice lies in its
// server's range), so every key is still applied once.
template <typename Value>
void KVWorker<Value>::Refused(const Message& msg) {
  const int ts = msg.meta.timestamp;
  ++refused_;
  SpecSend sp;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = spec_sends_.find(ts);
    CHECK(it != spec_sends_.end()) << "a refusal of request " << ts << ", which was not sent on unconfirmed slices";
    sp = it->second;
    spec_stale_[sp.kvs.keys.data()] = true;  // the sender's thread slices it for real next time
  }
  const int r = PostOffice::IDToRank(msg.meta.sender);
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  CHECK_LT((size_t)r + 1, sp.pos.size());
  std::vector<uint64_t> pos, vpos;
  device::SliceKeys(sp.kvs.keys.data(), sp.kvs.keys.size(), nullptr, sp.kvs.vals.size(), ranges, &pos, &vpos);
  int sent = 0;
  SendPieces(ts, sp, sp.pos[r], sp.pos[r + 1], pos, &sent);
  // (before this reply is counted: the request now waits for `sent` more)
  customer_->ExpectMore(ts, sent);
}

template <typename Value>
void KVWorker<Value>::SendPieces(int timestamp, const SpecSend& sp, uint64_t a, uint64_t b,
                                 const std::vector<uint64_t>& pos, int* sent) {
  const size_t n = sp.kvs.keys.size();
  const size_t per = n ? sp.kvs.vals.size() / n : 0;
  *sent = 0;
  for (size_t i = 0; i + 1 < pos.size(); ++i) {
    const uint64_t lo = std::max<uint64_t>(a, pos[i]), hi = std::min<uint64_t>(b, pos[i + 1]);
    if (lo >= hi) continue;
    Data kv;
    kv.keys = sp.kvs.keys.Slice(lo, hi);
    kv.vals = sp.kvs.vals.Slice(lo * per, hi * per);
    SendOne(timestamp, sp.push, sp.pull, sp.cmd, sp.kvs.priority, sp.kvs, kv, sp.direct,
            sp.has_outs ? &sp.outs : nullptr, (int)i, false);
    ++*sent;
  }
}

template <typename Value>
void KVWorker<Value>::OnReceive(const Message& msg) {
  if (msg.meta.simple_app) {
    SimpleApp::OnReceive(msg);
    return;
  }
  const int ts = msg.meta.timestamp;
  if (msg.meta.hbm_handle && !servers_take_hbm_.load()) NoteHbmServer(msg.meta.sender);
  if (msg.meta.spec_slice && !servers_take_spec_.load()) NoteSpecServer(msg.meta.sender);
  if (msg.meta.refused) {
    Refused(msg);
    return;  // (counted as a reply; the re-sent pieces are waited for)
  }
  if (msg.meta.pull) {
    CHECK_GE(msg.data.size(), (size_t)2);
    Reply r;
    r.kv.keys = msg.data[0];
    r.kv.vals = msg.data[1];
    if (msg.data.size() > 2) r.kv.lens = msg.data[2];
    r.sender = msg.meta.sender;
    r.direct = msg.meta.direct_reply;
    std::lock_guard<std::mutex> lk(mu_);
    recv_kvs_[ts].push_back(std::move(r));
  }
  // the tracker is bumped after this handle returns (Customer.cpp:58-67)
  if (customer_->GetResponse(ts) == customer_->NumExpected(ts) - 1) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      spec_sends_.erase(ts);
    }
    RunCallback(ts);
  }
}

template <typename Value>
void KVWorker<Value>::RunCallback(int timestamp) {
  Callback cb;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = callbacks_.find(timestamp);
    if (it == callbacks_.end()) return;
    cb = std::move(it->second);
    callbacks_.erase(it);
  }
  CHECK(static_cast<bool>(cb));
  cb();
}

template <typename Value>
template <typename C, typename D>
int KVWorker<Value>::AddPullCB(const SVector<Key>& keys, C* vals, D* lens, int cmd, const Callback& cb, bool routed) {
  (void)cmd;
  int ts = customer_->NewRequest(kServerGroup);
  AddCallback(ts, [this, ts, keys, vals, lens, cb, routed]() mutable {
    std::vector<Reply> kvs;
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = recv_kvs_.find(ts);
      if (it != recv_kvs_.end()) {
        kvs.swap(it->second);
        recv_kvs_.erase(it);
      }
    }
    MergePull(keys, kvs, vals, lens, routed);
    if (cb) cb();
  });
  return ts;
}

template <typename Value>
template <typename C, typename D>
void KVWorker<Value>::MergePull(const SVector<Key>& keys, std::vector<Reply>& kvs, C* vals, D* lens, bool routed) {
  stage::Scope t_merge("worker.pull.merge", keys.size() * sizeof(Value));
  size_t total_key = 0, total_val = 0;
  int ndev = 0, ndirect = 0;
  for (const auto& r : kvs) {
    const auto& s = r.kv;
    if (!routed && !s.keys.on_device() && !keys.on_device() && s.keys.size()) {
      Range range = FindRange(keys, s.keys.front(), s.keys.back() + 1);
      CHECK_EQ(range.size(), s.keys.size()) << "unmatched keys size from one server";
    }
    if (lens) CHECK_EQ(s.lens.size(), s.keys.size());
    total_key += s.keys.size();
    if (r.direct) {
      // written in place: its slice of the output, keys x values per key
      CHECK(!lens && vals && keys.size()) << "a direct reply needs a sized output and no lens";
      total_val += s.keys.size() * (vals->size() / keys.size());
      ++ndirect;
      continue;
    }
    total_val += s.vals.size();
    ndev += s.vals.on_device() ? 1 : 0;
  }
  CHECK_EQ(total_key, keys.size()) << "lost some servers?";
  CHECK(ndev == 0 || ndev + ndirect == (int)kvs.size()) << "pull replies mix host and HBM frames";
  // order the replies by their first key (KVApp.h:694-696); replies whose keys
  // are in HBM, and those of a routed list (each server's stretch is in arrival
  // order, not sorted), are ordered by server rank, which the default ranges
  // make the same
  if (!keys.on_device() && !routed) {
    std::sort(kvs.begin(), kvs.end(), [](const Reply& a, const Reply& b) {
      return a.kv.keys.front() < b.kv.keys.front();
    });
  } else {
    std::sort(kvs.begin(), kvs.end(), [](const Reply& a, const Reply& b) { return a.sender < b.sender; });
  }
  CHECK_NOTNULL(vals);
  const int out_dev = detail::DeviceOf(vals);
  if (vals->empty()) {
    CHECK_LT(out_dev, 0) << "an HBM pull output must be sized by the caller";
    stage::Scope t("worker.pull.merge.resize_output", total_val * sizeof(Value));
    // the reference resizes the caller's vector (KVApp.h:703-711); its fresh
    // pages are faulted in first, in parallel and on huge pages (PrefaultHost)
    // — a 40 MB reply's resize took 6.4-8 ms one 4 KiB fault at a time
    if (out_dev < 0) {
      vals->reserve(total_val);
      PrefaultHost(vals->data(), total_val * sizeof(Value));
    }
    vals->resize(total_val);
  } else {
    CHECK_EQ(vals->size(), total_val);
  }
  if (ndirect == (int)kvs.size()) {
    // every server wrote its values in place: nothing to merge
  } else if (ndev == 0 && out_dev < 0) {
    stage::Scope t("worker.pull.merge.copy", total_val * sizeof(Value));
    Value* p = vals->data();
    for (const auto& r : kvs) {
      if (r.kv.vals.size()) HostCopy(p, r.kv.vals.data(), r.kv.vals.size() * sizeof(Value));
      p += r.kv.vals.size();
    }
  } else if (total_val) {
    std::vector<psg_segment> segs;
    std::vector<SVector<Value>> staged;  // host replies going to an HBM output
    const int my_dev = PostOffice::Get()->device();
    const size_t per_key = keys.size() ? total_val / keys.size() : 0;
    std::vector<uint64_t> offs;  // where each segment goes in the output
    uint64_t done_vals = 0;      // values of the replies before j (direct ones included)
    for (size_t j = 0; j < kvs.size(); ++j) {
      if (kvs[j].direct) {
        done_vals += kvs[j].kv.keys.size() * per_key;
        continue;
      }
      const SVector<Value>& v = kvs[j].kv.vals;
      const Value* src = v.data();
      if (!v.on_device() && v.size()) {
        staged.push_back(detail::ToDevice(v, out_dev >= 0 ? out_dev : my_dev));
        src = staged.back().data();
      }
      segs.push_back(psg_segment{src, v.size(), (uint64_t)j});  // j: already in order
      offs.push_back(done_vals);
      done_vals += v.size();
    }
    if (out_dev >= 0 && ndirect == 0) {
      device::Merge(&segs, sizeof(Value), vals->data(), total_val);
    } else if (out_dev >= 0) {
      // some servers wrote in place: copy the other replies to their slices
      for (size_t t = 0; t < segs.size(); ++t) {
        std::vector<psg_segment> one{segs[t]};
        device::Merge(&one, sizeof(Value), vals->data() + offs[t], segs[t].count);
      }
    } else {
      SVector<Value> tmp = SVector<Value>::OnDevice(total_val, my_dev);
      device::Merge(&segs, sizeof(Value), tmp.data(), total_val);
      device::StageToHost(vals->data(), tmp.data(), total_val * sizeof(Value));
    }
  }
  if (lens) {
    CHECK_LT(detail::DeviceOf(lens), 0) << "pull lens are returned in host memory";
    if (lens->empty())
      lens->resize(keys.size());
    else
      CHECK_EQ(lens->size(), keys.size());
    int* p = lens->data();
    for (const auto& r : kvs) {
      SVector<int> hl = detail::ToHost(r.kv.lens);
      if (hl.size()) std::memcpy(p, hl.data(), hl.size() * sizeof(int));
      p += hl.size();
    }
  }
}

}  // namespace ps
