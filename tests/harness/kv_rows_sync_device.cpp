// kv_rows_sync_device.cpp — rows of W floats per key trained on the servers in
// sync-mode rounds, end to end through KVWorker / KVServer on the GPU data path
// (run by tests/test_rows_sync_dropin_gpu.py).
//
// The servers run KVServerRowSyncHandle(W, lr, adam) (ps/row_sync_handle.h: the
// sync-mode LRServer handle, tests/src/LRServer.h:151-178, on a psg_table in
// HBM).  All workers build the same list of distinct keys spread over the whole
// key range, so every server owns some.  Worker 0 seeds every row with a
// cmd = 2 (accumulate) Push.  Then, for rounds 0, 1, 2:
//   every worker Pushes gradients on an ascending list of its own — about half
//     of the keys, always the lowest and the highest, so every worker reaches
//     every server and the lists overlap — worker 0 with cmd = 1, and Waits:
//     the servers answer when all the round's Pushes are in;      barrier
//   every worker Pulls all keys.                                  barrier
// The gradient requests alternate between HBM frames (ZPush / ZPushPull) and
// host vectors (PushPull), so a PushPull's reply, the updated rows, is checked
// on both paths.
//
// Every worker replays every round on a host map: the gradients of all workers
// are merged per key from zero (f32 adds), then one update in plain C++
// (LRServer.h:167, Adam.h:28-34, the same operation order); every pulled value
// is compared bit for bit.  The servers merge in arrival order, which the
// harness does not control.  With up to 2 workers the gradients are real-valued:
// an f32 sum of two terms from zero does not depend on their order.  With more
// they are integer-valued (psg_fill_synth mode 0), so the sum is exact in any
// order.  No fused multiply-add may form in the replay: the harness rule of the
// Makefile compiles this file with -ffp-contract=off.
//
// On each server a wrapper around the handle checks iteration() after every
// gradient Push: it is the number of complete rounds (worker 0's cmd = 1 Push
// is in every round, and counts once the round is applied).
// Exits non-zero on the first mismatch.
// usage: kv_rows_sync_device [-ns S] [-nw W] [-procs] [width] [num_keys] [adam]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
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

static Row& RowOf(Rows& table, Key key, size_t w) {
  Row& r = table[key];
  if (r.w.empty()) {
    r.w.assign(w, 0.0f);
    r.m.assign(w, 0.0);
    r.v.assign(w, 0.0);
  }
  return r;
}

// one round of psg_table_update_merged: per key the frames' gradients summed
// from zero in the given order, then one update
static void ReplayRound(Rows& table, size_t w, const std::vector<std::vector<Key>>& keys,
                        const std::vector<std::vector<float>>& grads, bool adam, int iteration) {
  std::map<Key, std::vector<float>> merged;
  for (size_t f = 0; f < keys.size(); ++f)
    for (size_t i = 0; i < keys[f].size(); ++i) {
      auto& s = merged[keys[f][i]];
      if (s.empty()) s.assign(w, 0.0f);
      for (size_t j = 0; j < w; ++j) s[j] = s[j] + grads[f][i * w + j];
    }
  const double alr = (double)kLr;
  const double c1 = 1 - std::pow(kBeta1, iteration + 1);
  const double c2 = 1 - std::pow(kBeta2, iteration + 1);
  for (const auto& [key, s] : merged) {
    Row& r = RowOf(table, key, w);
    for (size_t j = 0; j < w; ++j) {
      double g = (double)(kLr * s[j]);
      if (adam) {
        r.m[j] = kBeta1 * r.m[j] + (1 - kBeta1) * g;
        r.v[j] = kBeta2 * r.v[j] + (1 - kBeta2) * g * g;
        g = alr * (r.m[j] / c1) / (std::sqrt(r.v[j] / c2) + kEps);
      }
      r.w[j] = (float)((double)r.w[j] - g);
    }
  }
}

static std::vector<float> ReplayPull(Rows& table, size_t w, const std::vector<Key>& keys) {
  std::vector<float> out(keys.size() * w);
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) out[i * w + j] = r.w[j];
  }
  return out;
}

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const char* what, int round) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << " of round " << round << ", value " << i << ": got " << got[i] << ", expected " << exp[i];
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 4 ? (size_t)std::atol(argv[4]) : 4;
  const size_t n = argc > 5 ? (size_t)std::atol(argv[5]) : 3000;
  const bool adam = argc > 6 ? std::atol(argv[6]) != 0 : true;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    KVServerRowSyncHandle handle((uint32_t)w, kLr, adam);
    auto pushes = std::make_shared<int>(0);
    const int nw = NumWorkers();
    server->SetDeviceRequestHandle(
        [handle, pushes, nw](const KVMeta& meta, const KVPairs<float>& data, KVServer<float>* s) mutable {
          handle(meta, data, s);
          if (meta.push && meta.cmd != KVServerRowSyncHandle::kAccumulate) {
            ++*pushes;
            CHECK_EQ(handle.iteration(), *pushes / nw) << "after gradient Push " << *pushes;
          }
        });
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const int nw = NumWorkers();
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
    // values: real in [-1, 1) for up to 2 workers, integers in [-8, 8) for more
    auto values = [&](size_t count, uint64_t seed) {
      auto d = SVector<float>::OnDevice(count * w, dev);
      psg_stream s = device::ThreadStream();
      device::Check(nw <= 2 ? psg_fill_synth(d.data(), count * w, PSG_F32, seed, 1, -1.0, 1.0, s)
                            : psg_fill_synth(d.data(), count * w, PSG_F32, seed, 0, -8.0, 8.0, s),
                    "psg_fill_synth");
      device::Check(psg_stream_sync(s), "psg_stream_sync");
      return to_host(d);
    };
    // the same n distinct keys over the whole key range on every worker
    std::mt19937_64 shared(99);
    std::vector<Key> all;
    while (all.size() < n) {
      for (size_t i = all.size(); i < n; ++i) all.push_back(shared() % kMaxKey);
      std::sort(all.begin(), all.end());
      all.erase(std::unique(all.begin(), all.end()), all.end());
    }
    Rows ref;

    const std::vector<float> seed = values(all.size(), 5);
    if (rank == 0) kv.Wait(kv.ZPush(to_dev(all), to_dev(seed), {}, KVServerRowSyncHandle::kAccumulate));
    for (size_t i = 0; i < all.size(); ++i) {
      Row& r = RowOf(ref, all[i], w);
      for (size_t j = 0; j < w; ++j) r.w[j] += seed[i * w + j];
    }
    Barrier(0, kWorkerGroup);

    for (int it = 0; it < 3; ++it) {
      // every worker's request of this round, on every worker (the replay needs them all)
      std::vector<std::vector<Key>> lists(nw);
      std::vector<std::vector<float>> grads(nw);
      for (int r = 0; r < nw; ++r) {
        std::mt19937_64 rng(1000 * (it + 1) + r);
        for (size_t i = 0; i < all.size(); ++i)
          if (i == 0 || i + 1 == all.size() || (rng() & 1)) lists[r].push_back(all[i]);
        grads[r] = values(lists[r].size(), 100 * (it + 1) + r);
      }
      const std::vector<Key>& sub = lists[rank];
      const std::vector<float>& g = grads[rank];
      const int cmd = rank == 0 ? 1 : 0;
      ReplayRound(ref, w, lists, grads, adam, it);
      if (it == 0) {
        kv.Wait(kv.ZPush(to_dev(sub), to_dev(g), {}, cmd));
      } else if (it == 1) {
        std::vector<float> outs;
        kv.Wait(kv.PushPull(sub, g, &outs, nullptr, cmd));
        Compare(outs, ReplayPull(ref, w, sub), "host PushPull", it);
      } else {
        auto dout = SVector<float>::OnDevice(sub.size() * w, dev);
        kv.Wait(kv.ZPushPull(to_dev(sub), to_dev(g), &dout, nullptr, cmd));
        Compare(to_host(dout), ReplayPull(ref, w, sub), "HBM PushPull", it);
      }
      Barrier(0, kWorkerGroup);
      auto dout = SVector<float>::OnDevice(all.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(all), &dout));
      Compare(to_host(dout), ReplayPull(ref, w, all), "Pull", it);
      Barrier(0, kWorkerGroup);
    }
    std::printf("rows sync ok: worker %d of %d, width %zu, %zu keys, %s\n", rank, nw, w, all.size(),
                adam ? "Adam" : "SGD");
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
