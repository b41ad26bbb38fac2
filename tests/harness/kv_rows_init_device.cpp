// kv_rows_init_device.cpp — row tables whose rows start from seeded initial
// values (SetInit on the three row handles, psg_table_set_init), sharded over
// the servers, end to end through KVWorker and KVServer on the GPU data path
// (run by tests/test_rows_init_dropin_gpu.py).
//
// Every server runs one of the three row handles and is given the SAME
// SetInit(kSeed, kLo, kHi) before its first request:
//   opt   KVServerRowOptHandle(W, lr, Adam, 0, any_order)
//   sync  KVServerRowSyncHandle(W, lr, Adam)
//   acc   KVServerRowHandle<float>(W, any_order)
// One worker.  Nothing seeds the rows: every id starts from its initial row, which
// the harness restates on the host (InitValue: Philox4x32-10 on the key, the
// column's block and the seed, as include/psg.h defines it).  The host map holds,
// per id, that row and zero moments until a Push names it.
//   unseen    a ZPullAny with kRowLookup of ids nobody has sent (shuffled, with
//             repeats) is the restated generator; ZPullPooled, ZPullPooledWeighted
//             and ZPullPooledMean of such ids are the replay on initial rows (per
//             server in arrival order from +0, the servers in rank order); nothing
//             of it inserts: a second lookup answers the same.
//   training  iteration `it` is one Push of about half of the ids (cmd 1: it ends
//             the iteration; the accumulate handle adds the values instead); an
//             id's first Push finds its initial row.  After every iteration a
//             kRowLookup of ALL ids equals the host map — trained rows and the
//             initial rows of the ids not yet sent.
//   phase save:    unseen; iterations 0-1; every server SaveModel(dir/shard-<rank>);
//                  the lookup of all ids into dir/mid; iterations 2-3, which name
//                  ids the files do not hold; the lookup into dir/final.
//   phase resume:  every server SetInit with the same triple, LoadModel of every
//                  saved shard; the lookup of all ids equals dir/mid; iterations
//                  2-3; the lookup equals dir/final: the resumed job on another
//                  number of servers is the uninterrupted one, byte for byte.
// The harness rule of the Makefile compiles this file with -ffp-contract=off.
// Exits non-zero on the first mismatch.
// usage: kv_rows_init_device [-ns S] [-nw 1] [-procs] handle width dir phase saved_ns
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "internal/device.h"
#include "ps/ps.h"

using namespace ps;

static constexpr float kLr = 0.01f;
static constexpr double kBeta1 = 0.9, kBeta2 = 0.999, kEps = 1e-8;
static constexpr uint64_t kSeed = 0xC0FFEE1234567890ull;
static constexpr float kLo = -0.05f, kHi = 0.075f;
static constexpr size_t kIds = 300;
static constexpr int kAllButScheduler = kServerGroup + kWorkerGroup;

// ---- the generator, restated ------------------------------------------------------
static void Philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

static float InitValue(Key key, size_t j) {
  uint32_t c[4] = {(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)(j / 4), 0u};
  Philox4x32_10(c, (uint32_t)kSeed, (uint32_t)(kSeed >> 32));
  const float u = (float)(c[j % 4] >> 8) * 0x1p-24f;
  const float span = kHi - kLo;
  const float prod = u * span;
  return kLo + prod;
}

struct Row {
  std::vector<float> w;
  std::vector<double> m, v;
};
using Rows = std::unordered_map<Key, Row>;

// the id's row in the host map: its initial row and zero moments until it was trained
static Row& RowOf(Rows& table, Key key, size_t w) {
  Row& r = table[key];
  if (r.w.empty()) {
    r.w.resize(w);
    for (size_t j = 0; j < w; ++j) r.w[j] = InitValue(key, j);
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

// a float in [-1, 1) from (a, key, column): splitmix64 of their mix
static float Value(uint64_t a, Key key, uint64_t col) {
  uint64_t z = key + 0x9e3779b97f4a7c15ull * (a * 1315423911ull + col + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (float)(z >> 40) / 8388608.0f - 1.0f;
}

static void WriteFile(const std::string& path, const std::vector<float>& v) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  f.write((const char*)v.data(), v.size() * sizeof(float));
  CHECK(f.good()) << "writing " << path;
}

static std::vector<float> ReadFile(const std::string& path, size_t count) {
  std::ifstream f(path, std::ios::binary);
  CHECK(f.is_open()) << path << " is missing";
  std::vector<float> v(count);
  f.read((char*)v.data(), count * sizeof(float));
  CHECK_EQ((size_t)f.gcount(), count * sizeof(float)) << path << " is too short";
  CHECK(f.peek() == EOF) << path << " is too long";
  return v;
}

static void Compare(const std::vector<float>& got, const std::vector<float>& exp, const std::string& what) {
  CHECK_EQ(got.size(), exp.size()) << what;
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << what << ", value " << i << ": got " << got[i] << ", expected " << exp[i];
  }
}

enum Pooling { kSum, kWeighted, kMean };

// the pooled forward on the host map, every id present or not: per bag, per server
// in rank order its ids in arrival order from +0, then the servers from +0; a mean
// divides the fold once by the bag's whole length
static std::vector<float> ReplayLookup(Rows& table, size_t w, const std::vector<Key>& keys,
                                       const std::vector<uint64_t>& offsets, const std::vector<float>& weights,
                                       Pooling pooling) {
  const size_t nb = offsets.size() - 1, ns = PostOffice::Get()->GetServerRanges().size();
  std::vector<float> out(nb * w);
  for (size_t b = 0; b < nb; ++b) {
    std::vector<float> acc(w, 0.0f);
    for (size_t s = 0; s < ns; ++s) {
      std::vector<float> part(w, 0.0f);
      for (uint64_t p = offsets[b]; p < offsets[b + 1]; ++p) {
        if (OwnerOf(keys[p]) != s) continue;
        const Row& r = RowOf(table, keys[p], w);
        for (size_t j = 0; j < w; ++j) {
          const float x = pooling == kWeighted ? weights[p] * r.w[j] : r.w[j];
          part[j] = part[j] + x;
        }
      }
      for (size_t j = 0; j < w; ++j) acc[j] = acc[j] + part[j];
    }
    const uint64_t len = offsets[b + 1] - offsets[b];
    for (size_t j = 0; j < w; ++j) out[b * w + j] = pooling == kMean ? (len ? acc[j] / (float)len : 0.0f) : acc[j];
  }
  return out;
}

template <typename Handle, typename Server>
static void ServerPhase(Handle handle, Server* server, const std::string& dir, const std::string& phase, int saved_ns) {
  handle.SetInit(kSeed, kLo, kHi);  // before the first request, the same triple on every server
  server->SetDeviceRequestHandle(handle);  // a copy: it shares the handle's state
  RegisterExitCallback([server]() { delete server; });
  if (phase == "save") {
    Barrier(0, kAllButScheduler);  // iterations 0-1 are applied and answered
    handle.SaveModel(dir + "/shard-" + std::to_string(MyRank()));
    Barrier(0, kAllButScheduler);
  } else {
    for (int r = 0; r < saved_ns; ++r) handle.LoadModel(dir + "/shard-" + std::to_string(r));
    Barrier(0, kAllButScheduler);
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  CHECK(argc > 8) << "usage: kv_rows_init_device handle width dir phase saved_ns";
  const std::string kind = argv[4];
  const size_t w = (size_t)std::atol(argv[5]);
  const std::string dir = argv[6];
  const std::string phase = argv[7];
  const int saved_ns = std::atoi(argv[8]);
  CHECK(kind == "opt" || kind == "sync" || kind == "acc") << kind;
  CHECK(phase == "save" || phase == "resume") << phase;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (kind == "opt")
      ServerPhase(KVServerRowOptHandle((uint32_t)w, kLr, true, 0, true), server, dir, phase, saved_ns);
    else if (kind == "sync")
      ServerPhase(KVServerRowSyncHandle((uint32_t)w, kLr, true), server, dir, phase, saved_ns);
    else
      ServerPhase(KVServerRowHandle<float>((uint32_t)w, true), server, dir, phase, saved_ns);
  }
  if (IsWorker()) {
    CHECK_EQ(NumWorkers(), 1) << "one worker";
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
    // the ids, over the whole key range; the lowest and the highest key among them
    std::mt19937_64 shared(99);
    std::vector<Key> ids = {0, kMaxKey - 1, (Key)1 << 32, ((Key)1 << 32) - 1};
    while (ids.size() < kIds) {
      for (size_t i = ids.size(); i < kIds; ++i) ids.push_back(shared() % kMaxKey);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    std::sort(ids.begin(), ids.end());
    Rows ref;
    int iteration = 0;
    // kRowLookup of a list (any order, repeats): nothing is inserted
    auto lookup = [&](const std::vector<Key>& list) {
      auto d = SVector<float>::OnDevice(list.size() * w, dev);
      kv.Wait(kv.ZPullAny(to_dev(list), &d, kRowLookup));
      return to_host(d);
    };
    auto expected = [&](const std::vector<Key>& list) {
      std::vector<float> exp(list.size() * w);
      for (size_t i = 0; i < list.size(); ++i) {
        const Row& r = RowOf(ref, list[i], w);
        std::copy(r.w.begin(), r.w.end(), exp.begin() + i * w);
      }
      return exp;
    };
    auto check_all = [&](const std::string& when) {
      std::vector<Key> every = ids;
      every.insert(every.end(), ids.begin(), ids.begin() + 20);  // repeats
      std::mt19937_64 ge(77);
      std::shuffle(every.begin(), every.end(), ge);
      Compare(lookup(every), expected(every), "kRowLookup of every id " + when);
      return lookup(ids);
    };
    auto check_pooled = [&](const std::string& when) {
      std::mt19937_64 g(5);
      std::vector<Key> keys(700);
      for (auto& k : keys) k = ids[g() % ids.size()];
      std::vector<uint64_t> offsets = {0, 0};
      while (offsets.back() < keys.size()) offsets.push_back(std::min<uint64_t>(keys.size(), offsets.back() + g() % 9));
      offsets.push_back(keys.size());
      std::vector<float> weights(keys.size());
      for (size_t i = 0; i < weights.size(); ++i) weights[i] = i % 8 ? Value(3, i, 0) : 0.0f;
      const size_t nb = offsets.size() - 1;
      auto dk = to_dev(keys);
      auto doff = to_dev(offsets);
      auto out = SVector<float>::OnDevice(nb * w, dev);
      kv.Wait(kv.ZPullPooled(dk, doff, &out));
      Compare(to_host(out), ReplayLookup(ref, w, keys, offsets, weights, kSum), "ZPullPooled " + when);
      kv.Wait(kv.ZPullPooledWeighted(dk, doff, to_dev(weights), &out));
      Compare(to_host(out), ReplayLookup(ref, w, keys, offsets, weights, kWeighted), "ZPullPooledWeighted " + when);
      kv.Wait(kv.ZPullPooledMean(dk, doff, &out));
      Compare(to_host(out), ReplayLookup(ref, w, keys, offsets, weights, kMean), "ZPullPooledMean " + when);
    };
    // iteration `it`: about half of the ids, ascending; an id's first Push finds its initial row
    auto train = [&](int it) {
      std::mt19937_64 rng(1000 * (it + 1));
      std::vector<Key> sub;
      for (size_t i = 0; i < ids.size(); ++i)
        if (i == 0 || i + 1 == ids.size() || (rng() & 1)) sub.push_back(ids[i]);
      std::vector<float> vals(sub.size() * w);
      for (size_t i = 0; i < sub.size(); ++i)
        for (size_t j = 0; j < w; ++j) vals[i * w + j] = Value(it + 1, sub[i], j);
      kv.Wait(kv.ZPush(to_dev(sub), to_dev(vals), {}, kind == "acc" ? 0 : 1));
      const double c1 = 1 - std::pow(kBeta1, iteration + 1), c2 = 1 - std::pow(kBeta2, iteration + 1);
      for (size_t i = 0; i < sub.size(); ++i) {
        Row& r = RowOf(ref, sub[i], w);
        for (size_t j = 0; j < w; ++j) {
          if (kind == "acc") {
            r.w[j] = r.w[j] + vals[i * w + j];
            continue;
          }
          double g = (double)(kLr * vals[i * w + j]);
          r.m[j] = kBeta1 * r.m[j] + (1 - kBeta1) * g;
          r.v[j] = kBeta2 * r.v[j] + (1 - kBeta2) * g * g;
          g = (double)kLr * (r.m[j] / c1) / (std::sqrt(r.v[j] / c2) + kEps);
          r.w[j] = (float)((double)r.w[j] - g);
        }
      }
      ++iteration;  // worker 0's cmd 1 ended the iteration on every server it reached: all of them
      check_all("after iteration " + std::to_string(it));
    };
    if (phase == "save") {
      // ids nobody has sent: the generator itself, at every server count
      std::vector<float> gen(ids.size() * w);
      for (size_t i = 0; i < ids.size(); ++i)
        for (size_t j = 0; j < w; ++j) gen[i * w + j] = InitValue(ids[i], j);
      Compare(check_all("before any Push"), gen, "unseen ids against the restated generator");
      check_pooled("of unseen ids");
      Compare(check_all("after the pooled lookups"), gen, "the lookups inserted nothing");
      train(0);
      train(1);
      check_pooled("of trained and unseen ids");
      Barrier(0, kAllButScheduler);
      Barrier(0, kAllButScheduler);  // the shards are written
      WriteFile(dir + "/mid", check_all("after the save"));
      train(2);
      train(3);
      WriteFile(dir + "/final", check_all("at the end"));
    } else {
      Barrier(0, kAllButScheduler);  // the shards are loaded
      // the host map of the resumed job is not the saved one's: the files are the reference here
      const std::vector<float> mid = lookup(ids);
      Compare(mid, ReadFile(dir + "/mid", ids.size() * w), "the resumed job's rows against dir/mid");
      auto quiet_train = [&](int it) {
        std::mt19937_64 rng(1000 * (it + 1));
        std::vector<Key> sub;
        for (size_t i = 0; i < ids.size(); ++i)
          if (i == 0 || i + 1 == ids.size() || (rng() & 1)) sub.push_back(ids[i]);
        std::vector<float> vals(sub.size() * w);
        for (size_t i = 0; i < sub.size(); ++i)
          for (size_t j = 0; j < w; ++j) vals[i * w + j] = Value(it + 1, sub[i], j);
        kv.Wait(kv.ZPush(to_dev(sub), to_dev(vals), {}, kind == "acc" ? 0 : 1));
      };
      quiet_train(2);
      quiet_train(3);
      Compare(lookup(ids), ReadFile(dir + "/final", ids.size() * w), "the resumed job's rows against dir/final");
    }
    std::printf("rows init %s ok: %s, width %zu, %zu ids, %d servers\n", phase.c_str(), kind.c_str(), w, ids.size(),
                NumServers());
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
