// kv_rows_bags_modes_device.cpp — the other two poolings of a bag on a table
// sharded over the servers, end to end through KVWorker::ZPullPooledWeighted /
// ZPushPooledWeighted / ZPullPooledMean / ZPushPooledMean / ZPushPooledMeanAll and
// KVServer on the GPU data path (run by tests/test_rows_bags_modes_dropin_gpu.py).
//
// mode 0: the servers run KVServerRowOptHandle(W, lr, true, 0, true): Adam and
//   any_order, as kv_rows_bags_device's mode 0, whose ids, seed and lists these
//   are, with one f32 weight per occurrence: one in eight is 0, the others lie in
//   [-1, 1) (half of them negative), and a hot id is named many times with a
//   different weight each time.  The workers take turns between barriers; in its
//   turn a worker sends ZPullPooledWeighted, ZPushPooledWeighted, ZPullPooledMean,
//   ZPushPooledMean and ZPullPooledMean again on one list (shuffled in most
//   turns, sorted — the identity route — in the others; bags of 0-12, the first
//   and the last empty).  Every other turn pushes with step = true (both Pushes).
//   Every worker replays every turn on a host map by the definitions of
//   include/psg.h ("Weighted and mean bags across servers"):
//     forward   per server in arrival order from +0 (weighted: one multiply, one
//               add per id), then the servers in rank order from +0, then for a
//               mean ONE division by the whole bag's length (an empty bag: +0);
//     backward  the whole-range E (weights[i] * grads[bag(i)], or grads[bag(i)] /
//               (float)L_bag(i)) summed per id from +0 in arrival order, then one
//               Adam step with the owner's iteration.
//   Every reply and a final ZPullAny of all rows are compared bit for bit.
// mode 1: KVServerRowSyncHandle(W, lr, true).  Two rounds; in each EVERY worker
//   sends ZPushPooledMeanAll with step on a list of its own.  The gradients are
//   integers (|value| <= 8) and the bags hold 0, 1, 2, 4 or 8 ids, so every E
//   value is a multiple of 1/8 and a merged sum does not depend on the order a
//   server took the workers' frames in.  The round's result is the host replay of
//   psg_table_update_pooled_merged on the expanded, divided rows; after each
//   round a weighted and a mean lookup of the worker's list are compared, and at
//   the end a ZPullAny of all rows.
// mode 2: the same handle; worker 0 sends one ZPushPooledWeighted, which the
//   handle must refuse with a CHECK before it is held.
// mode 3: KVServerRowHandle<float>(W, true): worker 0 seeds rows, its weighted and
//   mean lookups are compared with the replay, then its ZPushPooledWeighted must
//   fail RefusePooledUpdate's CHECK.
//
// The harness rule of the Makefile compiles this file with -ffp-contract=off.
// Exits non-zero on the first mismatch.
// usage: kv_rows_bags_modes_device [-ns S] [-nw W] [-procs] [width] [num_occurrences] [mode]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
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

// one list: occurrences in bags, a weight per occurrence, a gradient row per bag
struct List {
  std::vector<Key> keys;
  std::vector<uint64_t> offsets;
  std::vector<float> weights, grads;
};
enum Pooling { kWeighted, kMean };

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

// the forward: per bag, per server in rank order its present rows in arrival
// order from +0; a mean divides the fold once by the bag's whole length
static std::vector<float> ReplayLookup(const Rows& table, size_t w, const List& l, Pooling pooling) {
  const size_t nb = l.offsets.size() - 1, ns = PostOffice::Get()->GetServerRanges().size();
  std::vector<float> out(nb * w);
  for (size_t b = 0; b < nb; ++b) {
    std::vector<float> acc(w, 0.0f);
    for (size_t s = 0; s < ns; ++s) {
      std::vector<float> part(w, 0.0f);
      for (uint64_t p = l.offsets[b]; p < l.offsets[b + 1]; ++p) {
        auto it = table.find(l.keys[p]);
        if (OwnerOf(l.keys[p]) != s || it == table.end()) continue;
        for (size_t j = 0; j < w; ++j) {
          const float x = pooling == kWeighted ? l.weights[p] * it->second.w[j] : it->second.w[j];
          part[j] = part[j] + x;
        }
      }
      for (size_t j = 0; j < w; ++j) acc[j] = acc[j] + part[j];
    }
    const uint64_t len = l.offsets[b + 1] - l.offsets[b];
    for (size_t j = 0; j < w; ++j)
      out[b * w + j] = pooling == kMean ? (len ? acc[j] / (float)len : 0.0f) : acc[j];
  }
  return out;
}

// E of occurrence p in bag b, column j
static float Expanded(const List& l, Pooling pooling, size_t w, size_t b, uint64_t p, size_t j) {
  const float g = l.grads[b * w + j];
  return pooling == kWeighted ? l.weights[p] * g : g / (float)(l.offsets[b + 1] - l.offsets[b]);
}

// one update over frames: per id its E rows summed from +0, frames in order and
// occurrences in arrival order, then ONE Adam step with the owner's iteration
static void ReplayUpdate(Rows& table, size_t w, const std::vector<const List*>& frames, Pooling pooling,
                         const std::vector<int>& iteration) {
  std::unordered_map<Key, std::vector<float>> merged;
  std::vector<Key> order;
  for (const List* l : frames)
    for (size_t b = 0; b + 1 < l->offsets.size(); ++b)
      for (uint64_t p = l->offsets[b]; p < l->offsets[b + 1]; ++p) {
        auto& s = merged[l->keys[p]];
        if (s.empty()) {
          s.assign(w, 0.0f);
          order.push_back(l->keys[p]);
        }
        for (size_t j = 0; j < w; ++j) s[j] = s[j] + Expanded(*l, pooling, w, b, p, j);
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
  const size_t total = argc > 5 ? (size_t)std::atol(argv[5]) : 2000;
  const int mode = argc > 6 ? std::atoi(argv[6]) : 0;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (mode == 0)
      server->SetDeviceRequestHandle(KVServerRowOptHandle((uint32_t)w, kLr, true, 0, true));
    else if (mode == 3)
      server->SetDeviceRequestHandle(KVServerRowHandle<float>((uint32_t)w, true));
    else
      server->SetDeviceRequestHandle(KVServerRowSyncHandle((uint32_t)w, kLr, true));
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
    // a list of n occurrences (a few hot ids among them).  exact: bags of 0, 1, 2,
    // 4 or 8 ids and integer gradients (mode 1); else bags of 0-12 and real ones
    auto make_list = [&](uint64_t seed, size_t n, bool sorted, bool exact) {
      static const uint64_t kExactLen[5] = {0, 1, 2, 4, 8};
      std::mt19937_64 g(seed);
      List l;
      l.offsets = {0, 0};  // an empty first bag
      while (l.offsets.back() < n) {
        const uint64_t left = n - l.offsets.back();
        uint64_t len = exact ? kExactLen[g() % 5] : g() % 13;
        if (exact)
          while (len > left) len >>= 1;  // the cut at n keeps a power of two
        l.offsets.push_back(l.offsets.back() + std::min(len, left));
      }
      l.offsets.push_back(n);  // an empty last bag
      l.keys.resize(n);
      for (auto& k : l.keys) k = g() % 3 ? ids[g() % ids.size()] : ids[g() % 8 * 37];
      if (sorted) std::sort(l.keys.begin(), l.keys.end());
      l.weights = real_values(g, n);
      for (size_t i = 0; i < n; i += 8) l.weights[i] = 0.0f;
      l.grads.resize((l.offsets.size() - 1) * w);
      if (exact)
        for (auto& x : l.grads) x = (float)((int)(g() % 17) - 8);
      else
        l.grads = real_values(g, l.grads.size());
      return l;
    };
    // seed: five ids in six; the others are absent until an update names them
    Rows ref;
    std::vector<Key> seeded;
    for (size_t i = 0; i < ids.size(); ++i)
      if (i % 6) seeded.push_back(ids[i]);
    std::mt19937_64 gs(5);
    const std::vector<float> seed = real_values(gs, seeded.size() * w);
    auto seed_rows = [&](int cmd) {
      if (rank == 0) kv.Wait(kv.ZPushAny(to_dev(seeded), to_dev(seed), cmd));
      for (size_t i = 0; i < seeded.size(); ++i) {
        Row& r = RowOf(ref, seeded[i], w);
        for (size_t j = 0; j < w; ++j) r.w[j] += seed[i * w + j];
      }
      Barrier(0, kWorkerGroup);
    };
    // a weighted and a mean lookup of one list against the replay
    auto check_lookups = [&](const List& l, const char* when, int turn) {
      const size_t nb = l.offsets.size() - 1;
      auto dk = to_dev(l.keys);
      auto doff = to_dev(l.offsets);
      auto dout = SVector<float>::OnDevice(nb * w, dev);
      bool called = false;
      kv.Wait(kv.ZPullPooledWeighted(dk, doff, to_dev(l.weights), &dout, [&called]() { called = true; }));
      CHECK(called) << "Wait returned before the callback ran";
      Compare(to_host(dout), ReplayLookup(ref, w, l, kWeighted), (std::string("weighted Pull ") + when).c_str(), turn);
      auto dmean = SVector<float>::OnDevice(nb * w, dev);
      kv.Wait(kv.ZPullPooledMean(dk, doff, &dmean));
      Compare(to_host(dmean), ReplayLookup(ref, w, l, kMean), (std::string("mean Pull ") + when).c_str(), turn);
    };
    auto check_all_rows = [&]() {
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
    };

    if (mode == 2) {
      if (rank == 0) {
        const List l = make_list(1000, total, false, false);
        kv.Wait(kv.ZPushPooledWeighted(to_dev(l.keys), to_dev(l.offsets), to_dev(l.weights), to_dev(l.grads)));
        std::printf("rows bags modes: the sync handle took a weighted update\n");
        std::fflush(stdout);
      }
    } else if (mode == 3) {
      seed_rows(0);
      if (rank == 0) {
        const List l = make_list(1000, total, false, false);
        check_lookups(l, "on the accumulate handle", 0);
        std::printf("rows bags modes: the accumulate handle answered the weighted and the mean lookup\n");
        std::fflush(stdout);
        kv.Wait(kv.ZPushPooledWeighted(to_dev(l.keys), to_dev(l.offsets), to_dev(l.weights), to_dev(l.grads)));
        std::printf("rows bags modes: the accumulate handle took a weighted update\n");
        std::fflush(stdout);
      }
    } else if (mode == 1) {
      std::vector<int> iteration(ns, 0);
      seed_rows(KVServerRowSyncHandle::kAccumulate);
      const size_t n = std::max<size_t>(total / nw, 40);  // occurrences a worker sends in a round
      for (int round = 0; round < 2; ++round) {
        std::vector<List> lists;
        for (int r = 0; r < nw; ++r) lists.push_back(make_list(1000 + 16 * round + r, n, round == 1 && r == 0, true));
        std::vector<const List*> frames;
        for (const List& l : lists) frames.push_back(&l);
        const List& mine = lists[rank];
        bool called = false;
        kv.Wait(kv.ZPushPooledMeanAll(to_dev(mine.keys), to_dev(mine.offsets), to_dev(mine.grads), true,
                                      [&called]() { called = true; }));
        CHECK(called) << "Wait returned before the callback ran";
        ReplayUpdate(ref, w, frames, kMean, iteration);
        for (size_t s = 0; s < ns; ++s) ++iteration[s];  // worker 0's step ended an iteration on every server
        Barrier(0, kWorkerGroup);  // every worker's Wait has returned: the round is closed everywhere
        check_lookups(mine, "after the round", round);
        Barrier(0, kWorkerGroup);
      }
      check_all_rows();
      Barrier(0, kWorkerGroup);
      std::string line = "rows bags modes sync ok: worker " + std::to_string(rank) + ", width " + std::to_string(w) +
                         ", iterations";
      for (int it : iteration) line += " " + std::to_string(it);
      std::printf("%s\n", line.c_str());
      std::fflush(stdout);
    } else {
      std::vector<int> iteration(ns, 0);
      std::set<size_t> addressed;
      seed_rows(KVServerRowOptHandle::kAccumulate);
      const int rounds = 3;
      for (int round = 0; round < rounds; ++round)
        for (int r = 0; r < nw; ++r) {
          const int turn = round * nw + r;
          const bool step = turn % 2 == 0;
          const List l = make_list(1000 + turn, total, round == 1, false);
          const std::vector<const List*> frame = {&l};
          std::set<size_t> reached;
          for (Key k : l.keys) reached.insert(OwnerOf(k));
          auto end_step = [&]() {
            if (step && r == 0)
              for (size_t s : reached) ++iteration[s];
          };
          SVector<Key> dk;
          SVector<uint64_t> doff;
          SVector<float> dwt, dg;
          if (rank == r) {
            addressed.insert(reached.begin(), reached.end());
            dk = to_dev(l.keys);
            doff = to_dev(l.offsets);
            dwt = to_dev(l.weights);
            dg = to_dev(l.grads);
            check_lookups(l, "before the updates", turn);
            kv.Wait(kv.ZPushPooledWeighted(dk, doff, dwt, dg, step));
          }
          ReplayUpdate(ref, w, frame, kWeighted, iteration);
          end_step();
          if (rank == r) {
            check_lookups(l, "after the weighted update", turn);
            bool called = false;
            kv.Wait(kv.ZPushPooledMean(dk, doff, dg, step, [&called]() { called = true; }));
            CHECK(called) << "Wait returned before the callback ran";
          }
          ReplayUpdate(ref, w, frame, kMean, iteration);
          end_step();
          if (rank == r) {
            check_lookups(l, "after the mean update", turn);
            // the caller's arrays are as they were: the scaled frame is the worker's own
            Compare(to_host(dg), l.grads, "the caller's gradient rows after a mean Push", turn);
            Compare(to_host(dwt), l.weights, "the caller's weights after the turn", turn);
          }
          Barrier(0, kWorkerGroup);
        }
      check_all_rows();
      CHECK_EQ(ref.size(), ids.size()) << "the updates named every id";
      Barrier(0, kWorkerGroup);
      std::string line = "rows bags modes ok: worker " + std::to_string(rank) + ", width " + std::to_string(w) + ", " +
                         std::to_string(total) + " occurrences, iterations";
      for (int it : iteration) line += " " + std::to_string(it);
      line += ", servers addressed " + std::to_string(addressed.size());
      std::printf("%s\n", line.c_str());
      std::fflush(stdout);
    }
  }
  Finalize(0, true);
  return 0;
}
