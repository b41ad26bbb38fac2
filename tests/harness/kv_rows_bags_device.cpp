// kv_rows_bags_device.cpp — bags of ids on a table sharded over the servers, end
// to end through KVWorker::ZPullPooled / ZPushPooled and KVServer on the GPU data
// path (run by tests/test_rows_bags_dropin_gpu.py).
//
// mode 0: the servers run KVServerRowOptHandle(W, lr, true, 0, true): Adam, so a
//   row depends on the iteration it was updated in, and any_order, for the
//   final ZPullAny.  Worker 0 seeds most of the ids (cmd = 2); the others are
//   first seen by a pooled update, which inserts them.  Then the workers take
//   turns between barriers, so the servers' arrival order is fixed; in its turn
//   a worker sends ZPullPooled, ZPushPooled and ZPullPooled again on one list of
//   n occurrences of the shared ids in bags of 0-12, the first and the last bag
//   empty: shuffled in most turns, sorted (the identity route) in the others.
//   Every other turn pushes with step = true, which ends an iteration only when
//   worker 0 sends it, and only on the servers the list reaches.
//   Every worker replays every turn on a host map by the definition of
//   include/psg.h ("Bags across servers"): the forward adds a bag's rows per
//   server in arrival order from +0 and then the servers in rank order; the
//   backward sums, per id, the gradient rows of its bags in arrival order from
//   +0 and takes one Adam step with its server's iteration (Adam.h:28-34).  Every
//   pooled reply and a final ZPullAny of all rows are compared bit for bit.
// mode 1: the servers run KVServerRowHandle<float>(W, true); worker 0 sends one
//   ZPushPooled, whose cmd the accumulate handle must refuse with a CHECK.
//
// The harness rule of the Makefile compiles this file with -ffp-contract=off.
// Exits non-zero on the first mismatch.
// usage: kv_rows_bags_device [-ns S] [-nw W] [-procs] [width] [num_occurrences] [mode]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
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

// the backward: per id its bags' gradient rows summed in arrival order, one Adam step
static void ReplayUpdate(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<uint64_t>& offsets,
                         const std::vector<float>& grads, const std::vector<int>& iteration) {
  std::unordered_map<Key, std::vector<float>> merged;
  std::vector<Key> order;
  for (size_t b = 0; b + 1 < offsets.size(); ++b)
    for (uint64_t p = offsets[b]; p < offsets[b + 1]; ++p) {
      auto& s = merged[keys[p]];
      if (s.empty()) {
        s.assign(w, 0.0f);
        order.push_back(keys[p]);
      }
      for (size_t j = 0; j < w; ++j) s[j] = s[j] + grads[b * w + j];
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

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const char* what, int turn) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << ", turn " << turn << ", value " << i << ": got " << got[i] << ", expected " << exp[i];
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 4 ? (size_t)std::atol(argv[4]) : 4;
  const size_t n = argc > 5 ? (size_t)std::atol(argv[5]) : 2000;
  const int mode = argc > 6 ? std::atoi(argv[6]) : 0;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (mode == 1)
      server->SetDeviceRequestHandle(KVServerRowHandle<float>((uint32_t)w, true));
    else
      server->SetDeviceRequestHandle(KVServerRowOptHandle((uint32_t)w, kLr, true, 0, true));
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const int nw = NumWorkers();
    const int dev = PostOffice::Get()->device();
    const size_t ns = PostOffice::Get()->GetServerRanges().size();
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
    auto real_values = [&](std::mt19937_64& g, size_t count) {
      std::vector<float> v(count);
      for (auto& x : v) x = (float)((double)(g() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };
    // the same ids on every worker, over the whole key range
    std::mt19937_64 shared(99);
    std::vector<Key> ids;
    while (ids.size() < kIds) {
      for (size_t i = ids.size(); i < kIds; ++i) ids.push_back(shared() % kMaxKey);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    // one turn's list: n occurrences (a few hot ids among them) in bags of 0-12
    struct Turn {
      std::vector<Key> keys;
      std::vector<uint64_t> offsets;
      std::vector<float> grads;
    };
    auto make_turn = [&](int turn, bool sorted) {
      std::mt19937_64 g(1000 + turn);
      Turn t;
      t.offsets = {0, 0};  // an empty first bag
      while (t.offsets.back() < n) t.offsets.push_back(std::min<uint64_t>(n, t.offsets.back() + g() % 13));
      t.offsets.push_back(n);  // an empty last bag
      t.keys.resize(n);
      for (auto& k : t.keys) k = g() % 3 ? ids[g() % ids.size()] : ids[g() % 8 * 37];
      if (sorted) std::sort(t.keys.begin(), t.keys.end());
      t.grads = real_values(g, (t.offsets.size() - 1) * w);
      return t;
    };

    if (mode == 1) {
      if (rank == 0) {
        const Turn t = make_turn(0, false);
        kv.Wait(kv.ZPushPooled(to_dev(t.keys), to_dev(t.offsets), to_dev(t.grads)));
        std::printf("rows bags: the accumulate handle took a pooled update\n");
        std::fflush(stdout);
      }
    } else {
      Rows ref;
      std::vector<int> iteration(ns, 0);
      std::set<size_t> addressed;
      // seed: five ids in six; the others are absent until an update names them
      std::vector<Key> seeded;
      for (size_t i = 0; i < ids.size(); ++i)
        if (i % 6) seeded.push_back(ids[i]);
      std::mt19937_64 gs(5);
      const std::vector<float> seed = real_values(gs, seeded.size() * w);
      if (rank == 0) kv.Wait(kv.ZPushAny(to_dev(seeded), to_dev(seed), KVServerRowOptHandle::kAccumulate));
      for (size_t i = 0; i < seeded.size(); ++i) {
        Row& r = RowOf(ref, seeded[i], w);
        for (size_t j = 0; j < w; ++j) r.w[j] += seed[i * w + j];
      }
      Barrier(0, kWorkerGroup);
      const int rounds = 3;
      for (int round = 0; round < rounds; ++round)
        for (int r = 0; r < nw; ++r) {
          const int turn = round * nw + r;
          const bool step = turn % 2 == 0;
          const Turn t = make_turn(turn, round == 1);
          const size_t nb = t.offsets.size() - 1;
          std::set<size_t> reached;
          for (Key k : t.keys) reached.insert(OwnerOf(k));
          if (rank == r) {
            addressed.insert(reached.begin(), reached.end());
            auto dk = to_dev(t.keys);
            auto doff = to_dev(t.offsets);
            auto dg = to_dev(t.grads);
            auto dout = SVector<float>::OnDevice(nb * w, dev);
            bool called = false;
            kv.Wait(kv.ZPullPooled(dk, doff, &dout, [&called]() { called = true; }));
            CHECK(called) << "Wait returned before the callback ran";
            Compare(to_host(dout), ReplayLookup(ref, w, t.keys, t.offsets), "pooled Pull before the update", turn);
            kv.Wait(kv.ZPushPooled(dk, doff, dg, step));
          }
          ReplayUpdate(ref, w, t.keys, t.offsets, t.grads, iteration);
          if (step && r == 0)
            for (size_t s : reached) ++iteration[s];
          if (rank == r) {
            auto dout = SVector<float>::OnDevice(nb * w, dev);
            kv.Wait(kv.ZPullPooled(to_dev(t.keys), to_dev(t.offsets), &dout));
            Compare(to_host(dout), ReplayLookup(ref, w, t.keys, t.offsets), "pooled Pull after the update", turn);
          }
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
      CHECK_EQ(ref.size(), ids.size()) << "the updates named every id";
      Barrier(0, kWorkerGroup);
      std::printf("rows bags ok: worker %d, width %zu, %zu occurrences, iterations", rank, w, n);
      for (int it : iteration) std::printf(" %d", it);
      std::printf(", servers addressed %zu\n", addressed.size());
      std::fflush(stdout);
    }
  }
  Finalize(0, true);
  return 0;
}
