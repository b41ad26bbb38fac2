// kv_rows_opt_device.cpp — rows of W floats per key trained on the servers, end
// to end through KVWorker / KVServer on the GPU data path (run by
// tests/test_rows_opt_dropin_gpu.py).
//
// The servers run KVServerRowOptHandle(W, lr, adam) (ps/row_opt_handle.h: the
// async-mode LRServer handle, tests/src/LRServer.h:179-206, on a psg_table in
// HBM).  All workers build the same list of distinct keys spread over the whole
// key range, so every server owns some; worker r owns the keys of rank
// r mod nw and
//   seeds its rows with a cmd = 2 (accumulate) Push,
//   then for iterations 0, 1, 2:
//     every worker but worker 0 Pushes gradients on a subset of its keys and
//       Waits;                                   barrier
//     worker 0 does the same with cmd = 1, which ends the iteration on every
//       server its list reaches (it always holds its lowest and highest key);
//                                                barrier
//     every worker Pulls all its keys.
// The barriers make the iteration of every update deterministic.  The gradient
// requests alternate between HBM frames (ZPush / ZPushPull) and host vectors
// (PushPull), so a PushPull's reply is checked on both paths.
//
// Each request is replayed on a host map with the update's arithmetic in plain
// C++ (LRServer.h:182-189, Adam.h:28-34, the same operation order), and every
// pulled value is compared bit for bit.  No fused multiply-add may form in that
// replay: the harness rule of the Makefile compiles this file with
// -ffp-contract=off.  Exits non-zero on the first mismatch.
// usage: kv_rows_opt_device [-ns S] [-nw W] [-procs] [width] [num_keys] [adam]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static void ReplaySeed(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<float>& vals) {
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) r.w[j] += vals[i * w + j];
  }
}

// the update of psg_table_update; returns the updated rows (a PushPull's reply)
static std::vector<float> ReplayUpdate(Rows& table, size_t w, const std::vector<Key>& keys,
                                       const std::vector<float>& grads, bool adam, int iteration) {
  const double alr = (double)kLr;
  const double c1 = 1 - std::pow(kBeta1, iteration + 1);
  const double c2 = 1 - std::pow(kBeta2, iteration + 1);
  std::vector<float> out(keys.size() * w);
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) {
      double g = (double)(kLr * grads[i * w + j]);
      if (adam) {
        r.m[j] = kBeta1 * r.m[j] + (1 - kBeta1) * g;
        r.v[j] = kBeta2 * r.v[j] + (1 - kBeta2) * g * g;
        g = alr * (r.m[j] / c1) / (std::sqrt(r.v[j] / c2) + kEps);
      }
      r.w[j] = (float)((double)r.w[j] - g);
      out[i * w + j] = r.w[j];
    }
  }
  return out;
}

static std::vector<float> ReplayPull(Rows& table, size_t w, const std::vector<Key>& keys) {
  std::vector<float> out(keys.size() * w);
  for (size_t i = 0; i < keys.size(); ++i) {
    Row& r = RowOf(table, keys[i], w);
    for (size_t j = 0; j < w; ++j) out[i * w + j] = r.w[j];
  }
  return out;
}

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const char* what, int iteration) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << " of iteration " << iteration << ", value " << i << ": got " << got[i] << ", expected "
                   << exp[i];
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 4 ? (size_t)std::atol(argv[4]) : 4;
  const size_t n = argc > 5 ? (size_t)std::atol(argv[5]) : 3000;
  const bool adam = argc > 6 ? std::atol(argv[6]) != 0 : true;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    server->SetDeviceRequestHandle(KVServerRowOptHandle((uint32_t)w, kLr, adam));
    RegisterExitCallback([server]() { delete server; });
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
    // the same n distinct keys over the whole key range on every worker ...
    std::mt19937_64 shared(99);
    std::vector<Key> all;
    while (all.size() < n) {
      for (size_t i = all.size(); i < n; ++i) all.push_back(shared() % kMaxKey);
      std::sort(all.begin(), all.end());
      all.erase(std::unique(all.begin(), all.end()), all.end());
    }
    // ... of which this worker owns those of rank r mod nw
    std::vector<Key> mine;
    for (size_t i = (size_t)rank; i < all.size(); i += nw) mine.push_back(all[i]);
    std::mt19937_64 rng(1234 + rank);
    auto values = [&](size_t count) {
      std::vector<float> v(count * w);
      for (auto& x : v) x = (float)((double)(rng() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };
    Rows ref;

    const std::vector<float> seed = values(mine.size());
    kv.Wait(kv.ZPush(to_dev(mine), to_dev(seed), {}, KVServerRowOptHandle::kAccumulate));
    ReplaySeed(ref, w, mine, seed);
    Barrier(0, kWorkerGroup);

    for (int it = 0; it < 3; ++it) {
      // about half of this worker's keys, always its lowest and highest (so
      // worker 0's cmd = 1 Push reaches every server)
      std::vector<Key> sub;
      for (size_t i = 0; i < mine.size(); ++i)
        if (i == 0 || i + 1 == mine.size() || (rng() & 1)) sub.push_back(mine[i]);
      const std::vector<float> g = values(sub.size());
      auto push = [&](int cmd) {
        if (it == 0) {
          kv.Wait(kv.ZPush(to_dev(sub), to_dev(g), {}, cmd));
          ReplayUpdate(ref, w, sub, g, adam, it);
        } else if (it == 1) {
          std::vector<float> outs;
          kv.Wait(kv.PushPull(sub, g, &outs, nullptr, cmd));
          Compare(outs, ReplayUpdate(ref, w, sub, g, adam, it), "host PushPull", it);
        } else {
          auto dout = SVector<float>::OnDevice(sub.size() * w, dev);
          kv.Wait(kv.ZPushPull(to_dev(sub), to_dev(g), &dout, nullptr, cmd));
          Compare(to_host(dout), ReplayUpdate(ref, w, sub, g, adam, it), "HBM PushPull", it);
        }
      };
      if (rank != 0) push(0);
      Barrier(0, kWorkerGroup);
      if (rank == 0) push(1);
      Barrier(0, kWorkerGroup);
      auto dout = SVector<float>::OnDevice(mine.size() * w, dev);
      kv.Wait(kv.ZPull(to_dev(mine), &dout));
      Compare(to_host(dout), ReplayPull(ref, w, mine), "Pull", it);
    }
    std::printf("rows opt ok: worker %d, width %zu, %zu keys, %s\n", rank, w, mine.size(), adam ? "Adam" : "SGD");
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
