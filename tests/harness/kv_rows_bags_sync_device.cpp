// kv_rows_bags_sync_device.cpp — sync-mode rounds whose gradient frames are
// pooled, end to end through KVWorker::ZPushPooledAll, KVServerRowSyncHandle and
// psg_table_update_pooled_merged on the GPU data path (run by
// tests/test_rows_bags_sync_dropin_gpu.py).
//
// The servers run KVServerRowSyncHandle(W, lr, true): Adam, so a row depends on
// the iteration of every round that updated it.  Worker 0 seeds five ids in six
// (cmd = 2); the others are first seen by a round, which inserts them.  Then
// three rounds; in each, ALL workers send at once, every worker a list of its
// own of occurrences of the shared ids in bags of 0-12, the first and the last
// bag empty:
//   round 0: every worker sends ZPushPooledAll, worker 0 with step;
//   round 1: the same, and worker 0's list lies wholly inside server 0's range:
//            the other servers get its frame with zero keys, their rounds close
//            all the same and their iteration advances;
//   round 2: the last worker sends a plain ZPushPullAny (a gradient row per
//            occurrence) whose list reaches every server, the others pooled
//            Pushes; its reply is the updated rows.  (One worker: the round is
//            plain, and worker 0 ends the iteration with cmd 1.)
// The gradients are integer-valued (|value| <= 8), so a merged sum does not
// depend on the order a server took the workers' frames in.  Every worker
// replays every round on a host map — merge per id, then one Adam step with the
// server's iteration (LRServer.h:151-178, Adam.h:28-34) — and compares bit for
// bit: the plain reply, a ZPullPooled of its own list after each round, and a
// final ZPullAny(kRowLookup) of all ids.
//
// The harness rule of the Makefile compiles this file with -ffp-contract=off.
// Exits non-zero on the first mismatch.
// usage: kv_rows_bags_sync_device [-ns S] [-nw W] [-procs] [width] [num_occurrences]
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
static constexpr size_t kIds = 300;
static constexpr int kRounds = 3;

// one worker's frame of one round; plain: grads hold a row per occurrence and the
// offsets are used only by the pooled Pull that follows the round
struct Frame {
  std::vector<Key> keys;
  std::vector<uint64_t> offsets;
  std::vector<float> grads;
  bool plain = false;
};

static Row& RowOf(Rows& table, Key key, size_t w) {
  Row& r = table[key];
  if (r.w.empty()) {
    r.w.assign(w, 0.0f);
    r.m.assign(w, 0.0);
    r.v.assign(w, 0.0);
  }
  return r;
}

static size_t OwnerOf(Key k) {
  const std::vector<Range>& ranges = PostOffice::Get()->GetServerRanges();
  size_t s = 0;
  while (k >= ranges[s].end) ++s;
  return s;
}

// the forward: per bag, per server in rank order, its present rows in arrival order from +0
static std::vector<float> ReplayLookup(const Rows& table, size_t w, const std::vector<Key>& keys,
                                       const std::vector<uint64_t>& offsets) {
  const size_t nb = offsets.size() - 1, ns = PostOffice::Get()->GetServerRanges().size();
  std::vector<float> out(nb * w);
  for (size_t b = 0; b < nb; ++b) {
    std::vector<float> acc(w, 0.0f);
    for (size_t s = 0; s < ns; ++s) {
      std::vector<float> part(w, 0.0f);
      for (uint64_t p = offsets[b]; p < offsets[b + 1]; ++p) {
        auto it = table.find(keys[p]);
        if (OwnerOf(keys[p]) != s || it == table.end()) continue;
        for (size_t j = 0; j < w; ++j) part[j] = part[j] + it->second.w[j];
      }
      for (size_t j = 0; j < w; ++j) acc[j] = acc[j] + part[j];
    }
    std::copy(acc.begin(), acc.end(), out.begin() + b * w);
  }
  return out;
}

// one round: per id the gradient rows of all its occurrences in all frames summed
// from +0 (integers: any order gives the same sum), then ONE Adam step
static void ReplayRound(Rows& table, size_t w, const std::vector<Frame>& frames, const std::vector<int>& iteration) {
  std::unordered_map<Key, std::vector<float>> merged;
  std::vector<Key> order;
  auto add = [&](Key key, const float* g) {
    auto& s = merged[key];
    if (s.empty()) {
      s.assign(w, 0.0f);
      order.push_back(key);
    }
    for (size_t j = 0; j < w; ++j) s[j] = s[j] + g[j];
  };
  for (const Frame& f : frames) {
    if (f.plain) {
      for (size_t i = 0; i < f.keys.size(); ++i) add(f.keys[i], &f.grads[i * w]);
    } else {
      for (size_t b = 0; b + 1 < f.offsets.size(); ++b)
        for (uint64_t p = f.offsets[b]; p < f.offsets[b + 1]; ++p) add(f.keys[p], &f.grads[b * w]);
    }
  }
  const double alr = (double)kLr;
  for (Key key : order) {
    const int it = iteration[OwnerOf(key)];
    const double c1 = 1 - std::pow(kBeta1, it + 1);
    const double c2 = 1 - std::pow(kBeta2, it + 1);
    Row& r = RowOf(table, key, w);
    const std::vector<float>& s = merged[key];
    for (size_t j = 0; j < w; ++j) {
      double g = (double)(kLr * s[j]);
      r.m[j] = kBeta1 * r.m[j] + (1 - kBeta1) * g;
      r.v[j] = kBeta2 * r.v[j] + (1 - kBeta2) * g * g;
      g = alr * (r.m[j] / c1) / (std::sqrt(r.v[j] / c2) + kEps);
      r.w[j] = (float)((double)r.w[j] - g);
    }
  }
}

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const char* what, int round) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << ", round " << round << ", value " << i << ": got " << got[i] << ", expected " << exp[i];
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 4 ? (size_t)std::atol(argv[4]) : 4;
  const size_t total = argc > 5 ? (size_t)std::atol(argv[5]) : 2000;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    server->SetDeviceRequestHandle(KVServerRowSyncHandle((uint32_t)w, kLr, true));
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const int nw = NumWorkers();
    const int dev = PostOffice::Get()->device();
    const size_t ns = PostOffice::Get()->GetServerRanges().size();
    const size_t n = std::max<size_t>(total / nw, 40);  // occurrences a worker sends in a round
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
    // the same ids on every worker, over the whole key range
    std::mt19937_64 shared(99);
    std::vector<Key> ids;
    while (ids.size() < kIds) {
      for (size_t i = ids.size(); i < kIds; ++i) ids.push_back(shared() % kMaxKey);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    std::vector<std::vector<Key>> owned(ns);
    for (Key k : ids) owned[OwnerOf(k)].push_back(k);
    for (size_t s = 0; s < ns; ++s) CHECK(!owned[s].empty()) << "server " << s << " owns none of the ids";
    // worker r's frame of a round, the same on every worker (the replay needs them all)
    auto make_frame = [&](int round, int r) {
      std::mt19937_64 g(1000 + 16 * round + r);
      Frame f;
      f.plain = round == 2 && r == nw - 1;
      f.offsets = {0, 0};  // an empty first bag
      while (f.offsets.back() < n) f.offsets.push_back(std::min<uint64_t>(n, f.offsets.back() + g() % 13));
      f.offsets.push_back(n);  // an empty last bag
      const std::vector<Key>& from = round == 1 && r == 0 ? owned[0] : ids;
      f.keys.resize(n);
      for (auto& k : f.keys) k = g() % 3 ? from[g() % from.size()] : from[g() % 8 * (from.size() / 8)];
      if (f.plain)  // it reaches every server
        for (size_t s = 0; s < ns; ++s) f.keys[s] = owned[s][g() % owned[s].size()];
      std::shuffle(f.keys.begin(), f.keys.end(), g);
      f.grads.resize((f.plain ? n : f.offsets.size() - 1) * w);
      for (auto& x : f.grads) x = (float)((int)(g() % 17) - 8);
      return f;
    };

    Rows ref;
    std::vector<int> iteration(ns, 0);
    // seed: five ids in six; the others are absent until a round names them
    std::vector<Key> seeded;
    for (size_t i = 0; i < ids.size(); ++i)
      if (i % 6) seeded.push_back(ids[i]);
    std::mt19937_64 gs(5);
    std::vector<float> seed(seeded.size() * w);
    for (auto& x : seed) x = (float)((double)(gs() >> 11) * 0x1p-53 * 2.0 - 1.0);
    if (rank == 0) kv.Wait(kv.ZPushAny(to_dev(seeded), to_dev(seed), KVServerRowSyncHandle::kAccumulate));
    for (size_t i = 0; i < seeded.size(); ++i) {
      Row& r = RowOf(ref, seeded[i], w);
      for (size_t j = 0; j < w; ++j) r.w[j] += seed[i * w + j];
    }
    Barrier(0, kWorkerGroup);

    for (int round = 0; round < kRounds; ++round) {
      std::vector<Frame> frames;
      for (int r = 0; r < nw; ++r) frames.push_back(make_frame(round, r));
      const Frame& mine = frames[rank];
      if (round == 1)
        for (Key k : frames[0].keys) CHECK_EQ(OwnerOf(k), (size_t)0) << "round 1: worker 0's list stays on server 0";
      auto dk = to_dev(mine.keys);
      auto doff = to_dev(mine.offsets);
      auto dg = to_dev(mine.grads);
      SVector<float> reply;
      bool called = false;
      if (mine.plain) {
        reply = SVector<float>::OnDevice(n * w, dev);
        kv.Wait(kv.ZPushPullAny(dk, dg, &reply, rank == 0 ? 1 : 0, [&called]() { called = true; }));
      } else {
        kv.Wait(kv.ZPushPooledAll(dk, doff, dg, rank == 0, [&called]() { called = true; }));
      }
      CHECK(called) << "Wait returned before the callback ran";
      ReplayRound(ref, w, frames, iteration);
      for (size_t s = 0; s < ns; ++s) ++iteration[s];  // worker 0 ended an iteration on every server
      if (mine.plain) {
        std::vector<float> exp(n * w);
        for (size_t i = 0; i < n; ++i) {
          const Row& r = RowOf(ref, mine.keys[i], w);
          std::copy(r.w.begin(), r.w.end(), exp.begin() + i * w);
        }
        Compare(to_host(reply), exp, "the plain PushPull's reply", round);
      }
      // every server has answered this worker, so it has closed the round; the
      // barrier: every worker's Wait has returned, no Push of the round is under way
      Barrier(0, kWorkerGroup);
      auto dout = SVector<float>::OnDevice((mine.offsets.size() - 1) * w, dev);
      kv.Wait(kv.ZPullPooled(dk, doff, &dout));
      Compare(to_host(dout), ReplayLookup(ref, w, mine.keys, mine.offsets), "pooled Pull after the round", round);
      Barrier(0, kWorkerGroup);
    }
    // all rows, shuffled, unpooled
    std::vector<Key> every = ids;
    std::mt19937_64 ge(77 + rank);
    std::shuffle(every.begin(), every.end(), ge);
    auto dall = SVector<float>::OnDevice(every.size() * w, dev);
    kv.Wait(kv.ZPullAny(to_dev(every), &dall, kRowLookup));
    std::vector<float> exp(every.size() * w, 0.0f);
    for (size_t i = 0; i < every.size(); ++i) {
      auto it = ref.find(every[i]);
      if (it != ref.end()) std::copy(it->second.w.begin(), it->second.w.end(), exp.begin() + i * w);
    }
    Compare(to_host(dall), exp, "ZPullAny of all rows", -1);
    Barrier(0, kWorkerGroup);
    // one write: in a job of threads the workers print at the same time
    std::string line = "rows bags sync ok: worker " + std::to_string(rank) + ", width " + std::to_string(w) + ", " +
                       std::to_string(n * nw) + " occurrences a round, iterations";
    for (int it : iteration) line += " " + std::to_string(it);
    std::printf("%s\n", line.c_str());
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
