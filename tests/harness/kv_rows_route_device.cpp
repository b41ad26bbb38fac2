// kv_rows_route_device.cpp — key lists in any order and with repeats, routed to
// the servers that own their keys, on rows of W floats per key, end to end
// through KVWorker's Any calls and KVServer on the GPU data path (run by
// tests/test_rows_route_dropin_gpu.py).
//
// mode 0: the servers run KVServerRowHandle<float>(W, true) (any_order).
// mode 1: the servers run KVServerRowOptHandle(W, lr, false, 0, true) (SGD,
//   any_order; the seed is a cmd = 2 accumulate Push).
// mode 2: the servers run KVServerRowSyncHandle(W, lr, false): one sync-mode
//   round of overlapping shuffled lists, one from every worker.
//
// Modes 0 and 1.  Every worker sends, on keys of its own (key % nw == rank)
// drawn over the whole key space, so every server owns some:
//   ZPushAny / ZPushPullAny / ZPullAny of a shuffled list with repeats (HBM),
//   the same three of a sorted list with repeats (the identity route),
//   PushAny / PushPullAny / PullAny of another shuffled list as host vectors.
// Each request is replayed on a host map per occurrence in arrival order
// (src/ps/KVApp.h:446-454; mode 1: the update of tests/src/LRServer.h:182-189)
// and every pulled value is compared bit for bit.
//
// Mode 2.  Worker 0 seeds every row; every worker then sends one ZPushPullAny of
// a shuffled list with repeats that reaches every server (worker 0 with
// cmd = 1).  The round is replayed on the host as merge, then one update per
// key (LRServer.h:151-178); the gradients are integer-valued, so the merged sum
// does not depend on the order the servers took the frames in.  The reply and a
// ZPullAny of all keys, shuffled, are compared bit for bit.
//
// Each worker prints how many servers its lists addressed.  With `slicer` as the
// last argument the worker installs a custom slicer and then calls PushAny,
// whose CHECK must fail.  The harness rule of the Makefile compiles this file
// with -ffp-contract=off.  Exits non-zero on the first mismatch.
// usage: kv_rows_route_device [-ns S] [-nw W] [-procs] [width] [num_occurrences] [mode] [slicer]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <map>
#include <random>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "internal/device.h"
#include "ps/ps.h"

using namespace ps;

using Rows = std::unordered_map<Key, std::vector<float>>;

static constexpr float kLr = 0.01f;

// update == false: row += vals (KVApp.h:446-454); true: SGD (LRServer.h:182-189)
static std::vector<float> Replay(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<float>& vals,
                                 bool push, bool pull, bool update) {
  std::vector<float> out(pull ? keys.size() * w : 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    std::vector<float>& row = table[keys[i]];
    if (row.empty()) row.assign(w, 0.0f);
    for (size_t j = 0; j < w; ++j) {
      if (push && update) {
        const double g = (double)(kLr * vals[i * w + j]);
        row[j] = (float)((double)row[j] - g);
      } else if (push) {
        row[j] += vals[i * w + j];
      }
      if (pull) out[i * w + j] = row[j];
    }
  }
  return out;
}

// one sync-mode round: per key the frames' gradients summed from zero, then one SGD step
static void ReplayRound(Rows& table, size_t w, const std::vector<std::vector<Key>>& keys,
                        const std::vector<std::vector<float>>& grads) {
  std::map<Key, std::vector<float>> merged;
  for (size_t f = 0; f < keys.size(); ++f)
    for (size_t i = 0; i < keys[f].size(); ++i) {
      auto& s = merged[keys[f][i]];
      if (s.empty()) s.assign(w, 0.0f);
      for (size_t j = 0; j < w; ++j) s[j] = s[j] + grads[f][i * w + j];
    }
  for (const auto& [key, s] : merged) {
    std::vector<float>& row = table[key];
    if (row.empty()) row.assign(w, 0.0f);
    for (size_t j = 0; j < w; ++j) {
      const double g = (double)(kLr * s[j]);
      row[j] = (float)((double)row[j] - g);
    }
  }
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

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 4 ? (size_t)std::atol(argv[4]) : 4;
  const size_t n = argc > 5 ? (size_t)std::atol(argv[5]) : 3000;
  const int mode = argc > 6 ? std::atoi(argv[6]) : 0;
  const bool custom_slicer = argc > 7 && std::string(argv[7]) == "slicer";
  const bool opt = mode == 1;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (mode == 2)
      server->SetDeviceRequestHandle(KVServerRowSyncHandle((uint32_t)w, kLr, false));
    else if (opt)
      server->SetDeviceRequestHandle(KVServerRowOptHandle((uint32_t)w, kLr, false, 0, true));
    else
      server->SetDeviceRequestHandle(KVServerRowHandle<float>((uint32_t)w, true));
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const Key nw = (Key)NumWorkers();
    const int dev = PostOffice::Get()->device();
    KVWorker<float> kv(0, 0);
    std::mt19937_64 rng(8765 + rank);
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
    // the servers the lists sent so far addressed
    const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
    std::set<size_t> addressed;
    auto note = [&](const std::vector<Key>& keys) {
      for (Key k : keys)
        for (size_t s = 0; s < ranges.size(); ++s)
          if (k >= ranges[s].begin && k < ranges[s].end) addressed.insert(s);
    };
    auto real_values = [&](size_t count) {
      std::vector<float> v(count * w);
      for (auto& x : v) x = (float)((double)(rng() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };

    if (custom_slicer) {
      kv.set_slicer([](KVWorker<float>::Data& send, const std::vector<Range>& r, KVWorker<float>::SlicedKVs* sliced) {
        sliced->assign(r.size(), std::make_pair(false, KVWorker<float>::Data()));
        sliced->at(0) = std::make_pair(true, send);
      });
      const std::vector<Key> k{5, 3, 5};
      kv.Wait(kv.PushAny(k, real_values(k.size())));
      std::printf("rows route: the Any call passed a custom slicer\n");
      std::fflush(stdout);
    } else if (mode == 2) {
      // the same distinct keys over the whole key range on every worker
      std::mt19937_64 shared(99);
      std::vector<Key> all;
      while (all.size() < n / 4 + 2) {
        for (size_t i = all.size(); i < n / 4 + 2; ++i) all.push_back(shared() % kMaxKey);
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
      }
      auto int_values = [&](size_t count, uint64_t seed) {
        std::mt19937_64 g(seed);
        std::vector<float> v(count * w);
        for (auto& x : v) x = (float)((int)(g() % 16) - 8);
        return v;
      };
      Rows ref;
      const std::vector<float> seed = int_values(all.size(), 5);
      if (rank == 0) kv.Wait(kv.ZPush(to_dev(all), to_dev(seed), {}, KVServerRowSyncHandle::kAccumulate));
      Replay(ref, w, all, seed, true, false, false);
      Barrier(0, kWorkerGroup);
      // every worker's list, on every worker (the replay needs them all): n
      // occurrences, the lowest and the highest key among them, shuffled
      std::vector<std::vector<Key>> lists(nw);
      std::vector<std::vector<float>> grads(nw);
      for (Key r = 0; r < nw; ++r) {
        std::mt19937_64 g(1000 + r);
        lists[r] = {all.front(), all.back()};
        while (lists[r].size() < n) lists[r].push_back(all[g() % all.size()]);
        std::shuffle(lists[r].begin(), lists[r].end(), g);
        grads[r] = int_values(lists[r].size(), 100 + r);
      }
      ReplayRound(ref, w, lists, grads);
      const std::vector<Key>& mine = lists[rank];
      note(mine);
      auto dout = SVector<float>::OnDevice(mine.size() * w, dev);
      kv.Wait(kv.ZPushPullAny(to_dev(mine), to_dev(grads[rank]), &dout, rank == 0 ? 1 : 0));
      Compare(to_host(dout), Replay(ref, w, mine, {}, false, true, false), "routed PushPull of the round");
      Barrier(0, kWorkerGroup);
      std::vector<Key> every = all;
      std::shuffle(every.begin(), every.end(), rng);
      auto dall = SVector<float>::OnDevice(every.size() * w, dev);
      kv.Wait(kv.ZPullAny(to_dev(every), &dall));
      Compare(to_host(dall), Replay(ref, w, every, {}, false, true, false), "routed Pull after the round");
      Barrier(0, kWorkerGroup);
    } else {
      // `count` distinct ascending keys of this worker over the whole key space
      // (so every server owns some), none of them in `avoid`
      auto fresh_keys = [&](size_t count, const std::vector<Key>& avoid) {
        std::vector<Key> k;
        while (k.size() < count) {
          for (size_t i = k.size(); i < count; ++i) k.push_back(rng() % (kMaxKey / nw - 1) * nw + (Key)rank);
          std::sort(k.begin(), k.end());
          k.erase(std::unique(k.begin(), k.end()), k.end());
          std::vector<Key> kept;
          std::set_difference(k.begin(), k.end(), avoid.begin(), avoid.end(), std::back_inserter(kept));
          k.swap(kept);
        }
        return k;
      };
      // `count` occurrences drawn from `from` (each key about count / from.size() times)
      auto occurrences = [&](size_t count, const std::vector<Key>& from, bool shuffled) {
        std::vector<Key> k(count);
        for (auto& x : k) x = from[rng() % from.size()];
        if (shuffled)
          std::shuffle(k.begin(), k.end(), rng);
        else
          std::sort(k.begin(), k.end());
        return k;
      };
      const int cmd = 0;
      Rows ref;

      // ---- seed (mode 1): an accumulate Push, routed -----------------------------------
      const std::vector<Key> da = fresh_keys(n / 4 + 1, {});
      if (opt) {
        const std::vector<Key> s = occurrences(n, da, true);
        const std::vector<float> vs = real_values(s.size());
        note(s);
        kv.Wait(kv.ZPushAny(to_dev(s), to_dev(vs), KVServerRowOptHandle::kAccumulate));
        Replay(ref, w, s, vs, true, false, false);
      }

      // ---- HBM frames: shuffled with repeats, then sorted with repeats -------------------
      for (int sorted = 0; sorted < 2; ++sorted) {
        const char* what = sorted ? "sorted HBM list" : "shuffled HBM list";
        const std::vector<Key> a = occurrences(n, da, !sorted);
        const std::vector<float> va = real_values(n);
        note(a);
        auto dk = to_dev(a);
        auto dv = to_dev(va);
        kv.Wait(kv.ZPushAny(dk, dv, cmd));
        Replay(ref, w, a, va, true, false, opt);
        auto dout = SVector<float>::OnDevice(n * w, dev);
        bool called = false;
        kv.Wait(kv.ZPushPullAny(dk, dv, &dout, cmd, [&called]() { called = true; }));
        CHECK(called) << what << ": Wait returned before the callback ran";
        Compare(to_host(dout), Replay(ref, w, a, va, true, true, opt), what);
        auto dout2 = SVector<float>::OnDevice(n * w, dev);
        kv.Wait(kv.ZPullAny(dk, &dout2));
        Compare(to_host(dout2), Replay(ref, w, a, va, false, true, opt), what);
        // the caller's keys and values are as they were
        CHECK(to_host(dv) == va) << what << ": the caller's values changed";
      }

      // ---- host vectors: the first list's keys mixed with new ones, shuffled -------------
      std::vector<Key> db;
      for (size_t i = 0; i < da.size(); i += 2) db.push_back(da[i]);
      for (Key k : fresh_keys(n / 8 + 1, da)) db.push_back(k);
      std::sort(db.begin(), db.end());
      const std::vector<Key> b = occurrences(n, db, true);
      const std::vector<float> vb = real_values(b.size());
      note(b);
      kv.Wait(kv.PushAny(b, vb, cmd));
      Replay(ref, w, b, vb, true, false, opt);
      std::vector<float> outs;
      kv.Wait(kv.PushPullAny(b, vb, &outs, cmd));
      Compare(outs, Replay(ref, w, b, vb, true, true, opt), "host PushPullAny");
      std::vector<float> pulled;
      kv.Wait(kv.PullAny(b, &pulled));
      Compare(pulled, Replay(ref, w, b, vb, false, true, opt), "host PullAny");
      // a shuffled HBM Pull of everything: rows moved and were pushed to since
      std::vector<Key> every = da;
      every.insert(every.end(), db.begin(), db.end());
      std::shuffle(every.begin(), every.end(), rng);
      auto dall = SVector<float>::OnDevice(every.size() * w, dev);
      kv.Wait(kv.ZPullAny(to_dev(every), &dall));
      Compare(to_host(dall), Replay(ref, w, every, {}, false, true, opt), "shuffled HBM Pull after the inserts");
    }
    if (!custom_slicer) {
      std::printf("rows route ok: worker %d, width %zu, %zu occurrences, mode %d, servers addressed %zu\n", rank, w, n,
                  mode, addressed.size());
      std::fflush(stdout);
    }
  }
  Finalize(0, true);
  return 0;
}
