// kv_rows_lifecycle_device.cpp — rows read without inserting them (a Pull with
// cmd = kRowLookup) and rows erased (a Push with cmd = kRowErase and no values),
// end to end through KVWorker / KVServer on the GPU data path (run by
// tests/test_rows_lifecycle_dropin_gpu.py).
//
// The servers run one of
//   opt   KVServerRowOptHandle(W, lr, Adam)
//   acc   KVServerRowHandle<float>(W)          a "gradient" Push is a plain add
// All workers build the same list of distinct keys spread over the whole key
// range; worker r owns the keys of rank r mod nw, and ids of its own that no
// worker ever trains (`unseen`, `never`).  Every request is replayed on a host
// map — the update in plain C++ (LRServer.h:182-189, Adam.h:28-34; the Makefile
// compiles this file with -ffp-contract=off), a lookup that does not insert, an
// erase that drops the entry — and every pulled value is compared bit for bit.
//
//   1  seed, iterations 0 and 1 (worker 0's Push with cmd = 1 last, between
//      barriers, so every update's iteration is deterministic)        size "trained"
//   2  a lookup of a list that is half unseen ids: as ZPull, as host Pull, and
//      as ZPullAny on the list shuffled and with repeats              size "looked"
//      the same list as a plain Pull: it inserts the unseen ids       size "pulled"
//   3  four disjoint lists of present keys erased: Push and ZPush (ascending),
//      PushAny and ZPushAny (shuffled, with repeats and ids never present)
//                                                                     size "erased"
//      a lookup of the erased keys answers zeros; iteration 2 pushes every
//      erased key again, which the replay starts from a fresh row; a Pull of all
//      of the worker's keys equals the replay.
// At each `size` point every server prints its handle's size(); each worker
// prints the counts the test needs to check their sums.  With `badcmd` as the
// last argument worker 0 sends a PushPull with cmd = kRowErase instead: the
// server's CHECK ends the job.  Exits non-zero on the first mismatch.
// usage: kv_rows_lifecycle_device [-ns S] [-nw W] [-procs] handle [width] [num_keys] [badcmd]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "internal/device.h"
#include "ps/ps.h"

using namespace ps;

struct Row {
  std::vector<float> w;
  std::vector<double> m, v;
};
using Rows = std::unordered_map<Key, Row>;

static constexpr float kLr = 0.01f;
static constexpr double kBeta1 = 0.9, kBeta2 = 0.999, kEps = 1e-8;
static constexpr int kAllButScheduler = kServerGroup + kWorkerGroup;
static const char* const kPoints[] = {"trained", "looked", "pulled", "erased"};

static Row& RowOf(Rows& table, Key key, size_t w) {
  Row& r = table[key];
  if (r.w.empty()) {
    r.w.assign(w, 0.0f);
    r.m.assign(w, 0.0);
    r.v.assign(w, 0.0);
  }
  return r;
}

static void ReplayAdd(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<float>& vals) {
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) r.w[j] += vals[i * w + j];
  }
}

// the Adam update of psg_table_update
static void ReplayUpdate(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<float>& grads,
                         int iteration) {
  const double alr = (double)kLr;
  const double c1 = 1 - std::pow(kBeta1, iteration + 1);
  const double c2 = 1 - std::pow(kBeta2, iteration + 1);
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) {
      double g = (double)(kLr * grads[i * w + j]);
      r.m[j] = kBeta1 * r.m[j] + (1 - kBeta1) * g;
      r.v[j] = kBeta2 * r.v[j] + (1 - kBeta2) * g * g;
      g = alr * (r.m[j] / c1) / (std::sqrt(r.v[j] / c2) + kEps);
      r.w[j] = (float)((double)r.w[j] - g);
    }
  }
}

// a Pull: with `insert` an absent key becomes a zero row, as operator[] does
static std::vector<float> ReplayRead(Rows& table, size_t w, const std::vector<Key>& keys, bool insert) {
  std::vector<float> out(keys.size() * w, 0.0f);
  for (size_t i = 0; i < keys.size(); ++i) {
    if (!insert && !table.count(keys[i])) continue;
    const Row& r = RowOf(table, keys[i], w);
    std::copy(r.w.begin(), r.w.end(), out.begin() + i * w);
  }
  return out;
}

static size_t ReplayErase(Rows& table, const std::vector<Key>& keys) {
  size_t gone = 0;
  for (Key k : keys) gone += table.erase(k);
  return gone;
}

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const char* what) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << ", value " << i << ": got " << got[i] << ", expected " << exp[i];
  }
}

// the server's side: at each point, between two barriers, the rows it holds
template <typename Handle>
static void ServerSide(Handle handle, KVServer<float>* server, bool bad) {
  server->SetDeviceRequestHandle(handle);  // a copy: it shares the handle's state
  RegisterExitCallback([server]() { delete server; });
  if (bad) return;
  for (const char* point : kPoints) {
    Barrier(0, kAllButScheduler);  // the workers' requests up to here are answered
    std::printf("rows lifecycle size %s server %d: %zu\n", point, MyRank(), handle.size());
    std::fflush(stdout);
    Barrier(0, kAllButScheduler);
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  CHECK(argc > 4) << "usage: kv_rows_lifecycle_device handle [width] [num_keys] [badcmd]";
  const std::string kind = argv[4];
  const size_t w = argc > 5 ? (size_t)std::atol(argv[5]) : 4;
  const size_t n = argc > 6 ? (size_t)std::atol(argv[6]) : 2000;
  const bool bad = argc > 7 && std::string(argv[7]) == "badcmd";
  CHECK(kind == "opt" || kind == "acc") << kind;
  const bool opt = kind == "opt";
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (opt)
      ServerSide(KVServerRowOptHandle((uint32_t)w, kLr, true), server, bad);
    else
      ServerSide(KVServerRowHandle<float>((uint32_t)w), server, bad);
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const size_t nw = (size_t)NumWorkers();
    const int dev = PostOffice::Get()->device();
    KVWorker<float> kv(0, 0);
    auto to_dev = [&](const auto& v) {
      using T = typename std::decay_t<decltype(v)>::value_type;
      auto d = SVector<T>::OnDevice(v.size(), dev);
      device::CopySync(d.data(), v.data(), v.size() * sizeof(T), 0);
      return d;
    };
    auto to_host = [&](const SVector<float>& d) {
      std::vector<float> h(d.size());
      device::CopySync(h.data(), d.data(), d.size() * sizeof(float), 1);
      return h;
    };
    auto point = [&]() {  // the servers print their sizes between the two
      Barrier(0, kAllButScheduler);
      Barrier(0, kAllButScheduler);
    };
    // the same distinct keys over the whole key range on every worker: the
    // first n are trained (worker r owns those of rank r mod nw), the rest are
    // ids nobody trains (split among the workers the same way)
    const size_t extra = n;
    std::mt19937_64 shared(99);
    std::vector<Key> pool;
    while (pool.size() < n + extra) {
      for (size_t i = pool.size(); i < n + extra; ++i) pool.push_back(shared() % kMaxKey);
      std::sort(pool.begin(), pool.end());
      pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
    }
    std::shuffle(pool.begin(), pool.end(), shared);
    std::vector<Key> all(pool.begin(), pool.begin() + n), rest(pool.begin() + n, pool.end());
    std::sort(all.begin(), all.end());
    std::sort(rest.begin(), rest.end());
    std::vector<Key> mine, unseen, never;
    for (size_t i = (size_t)rank; i < all.size(); i += nw) mine.push_back(all[i]);
    for (size_t i = (size_t)rank; i < rest.size(); i += nw) (i / nw % 2 ? never : unseen).push_back(rest[i]);
    CHECK_GE(mine.size(), (size_t)16);
    std::mt19937_64 rng(1234 + rank);
    auto values = [&](size_t count) {
      std::vector<float> v(count * w);
      for (auto& x : v) x = (float)((double)(rng() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };
    auto sorted_union = [](std::vector<Key> a, const std::vector<Key>& b) {
      a.insert(a.end(), b.begin(), b.end());
      std::sort(a.begin(), a.end());
      return a;
    };
    // a list shuffled, with a tenth of it named again
    auto shuffled = [&](std::vector<Key> v) {
      const size_t k = v.size();
      for (size_t i = 0; i < k / 10 + 1; ++i) v.push_back(v[rng() % k]);
      std::shuffle(v.begin(), v.end(), rng);
      return v;
    };
    Rows ref;
    const int seed_cmd = opt ? KVServerRowOptHandle::kAccumulate : 0;

    if (bad) {
      if (rank == 0) {
        std::vector<float> outs;
        kv.Wait(kv.PushPull(mine, values(mine.size()), &outs, nullptr, kRowErase));
        std::printf("rows lifecycle: a PushPull passed with kRowErase\n");
        std::fflush(stdout);
      }
      Finalize(0, true);
      return 0;
    }

    // one iteration: every worker but worker 0, then worker 0 with cmd = 1
    auto train = [&](int it, const std::vector<Key>& sub) {
      const std::vector<float> g = values(sub.size());
      auto push = [&](int cmd) {
        if (it % 2)
          kv.Wait(kv.Push(sub, g, {}, opt ? cmd : 0));
        else
          kv.Wait(kv.ZPush(to_dev(sub), to_dev(g), {}, opt ? cmd : 0));
        if (opt)
          ReplayUpdate(ref, w, sub, g, it);
        else
          ReplayAdd(ref, w, sub, g);
      };
      if (rank != 0) push(0);
      Barrier(0, kWorkerGroup);
      if (rank == 0) push(1);
      Barrier(0, kWorkerGroup);
    };
    // about half of a list, always its lowest and highest key (so worker 0's
    // cmd = 1 Push reaches every server)
    auto half_of = [&](const std::vector<Key>& v) {
      std::vector<Key> sub;
      for (size_t i = 0; i < v.size(); ++i)
        if (i == 0 || i + 1 == v.size() || (rng() & 1)) sub.push_back(v[i]);
      return sub;
    };

    // ---- 1: seed and train --------------------------------------------------------
    const std::vector<float> seed = values(mine.size());
    kv.Wait(kv.ZPush(to_dev(mine), to_dev(seed), {}, seed_cmd));
    ReplayAdd(ref, w, mine, seed);
    Barrier(0, kWorkerGroup);
    train(0, half_of(mine));
    train(1, half_of(mine));
    point();  // trained

    // ---- 2: lookups leave the table alone, a plain Pull does not --------------------
    std::vector<Key> half;
    for (size_t i = 0; i < mine.size(); i += 2) half.push_back(mine[i]);
    const std::vector<Key> list = sorted_union(half, unseen);
    {
      auto dout = SVector<float>::OnDevice(list.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(list), &dout, nullptr, kRowLookup));
      Compare(to_host(dout), ReplayRead(ref, w, list, false), "lookup ZPull");
      std::vector<float> out;
      kv.Wait(kv.Pull(list, &out, nullptr, kRowLookup));
      Compare(out, ReplayRead(ref, w, list, false), "lookup Pull");
      const std::vector<Key> mixed = shuffled(list);
      auto dany = SVector<float>::OnDevice(mixed.size() * w, dev);
      kv.Wait(kv.ZPullAny(to_dev(mixed), &dany, kRowLookup));
      Compare(to_host(dany), ReplayRead(ref, w, mixed, false), "lookup ZPullAny");
    }
    point();  // looked
    {
      std::vector<float> out;
      kv.Wait(kv.Pull(list, &out));
      Compare(out, ReplayRead(ref, w, list, true), "plain Pull");
    }
    point();  // pulled

    // ---- 3: erase --------------------------------------------------------------------
    // four disjoint lists of this worker's keys; its lowest and highest key stay
    std::vector<Key> e[4];
    for (size_t i = 1; i + 1 < mine.size(); ++i)
      if (i % 2) e[i / 2 % 4].push_back(mine[i]);
    e[1].insert(e[1].end(), unseen.begin(), unseen.begin() + unseen.size() / 2);  // present since the plain Pull
    std::sort(e[1].begin(), e[1].end());
    const std::vector<Key> any2 = shuffled(sorted_union(e[2], never));
    const std::vector<Key> any3 = shuffled(sorted_union(e[3], never));
    size_t erased = 0;
    kv.Wait(kv.Push(e[0], {}, {}, kRowErase));
    erased += ReplayErase(ref, e[0]);
    kv.Wait(kv.ZPush(to_dev(e[1]), SVector<float>(), {}, kRowErase));
    erased += ReplayErase(ref, e[1]);
    kv.Wait(kv.PushAny(any2, {}, kRowErase));
    erased += ReplayErase(ref, any2);
    kv.Wait(kv.ZPushAny(to_dev(any3), SVector<float>(), kRowErase));
    erased += ReplayErase(ref, any3);
    CHECK_EQ(erased, e[0].size() + e[1].size() + e[2].size() + e[3].size());
    point();  // erased
    std::vector<Key> gone = sorted_union(sorted_union(e[0], e[1]), sorted_union(e[2], e[3]));
    {
      auto dout = SVector<float>::OnDevice(gone.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(gone), &dout, nullptr, kRowLookup));
      Compare(to_host(dout), std::vector<float>(gone.size() * w, 0.0f), "lookup of the erased keys");
      // and the survivors, with the erased keys among them
      auto dall = SVector<float>::OnDevice(mine.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(mine), &dall, nullptr, kRowLookup));
      Compare(to_host(dall), ReplayRead(ref, w, mine, false), "lookup after the erase");
    }
    Barrier(0, kWorkerGroup);
    // every erased key is pushed again, with survivors around it: the replay
    // starts it from a zero row and zero moments
    std::vector<Key> again = sorted_union(gone, {mine.front(), mine.back()});
    for (size_t i = 4; i + 1 < mine.size(); i += 4) again.push_back(mine[i]);
    std::sort(again.begin(), again.end());
    train(2, again);
    {
      auto dout = SVector<float>::OnDevice(mine.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(mine), &dout));
      Compare(to_host(dout), ReplayRead(ref, w, mine, true), "Pull after the erase");
    }
    std::printf("rows lifecycle ok: worker %d, %s, width %zu, keys %zu, unseen %zu, erased %zu\n", rank, kind.c_str(), w,
                mine.size(), unseen.size(), erased);
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
