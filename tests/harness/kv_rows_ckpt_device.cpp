// kv_rows_ckpt_device.cpp — a trained row table saved, loaded by another job on
// another number of servers, and trained on: the resumed job must pull, byte for
// byte, what the uninterrupted one pulled (run by
// tests/test_rows_ckpt_dropin_gpu.py).
//
// The servers run one of the three row handles, each with SaveModel / LoadModel
// (ps/row_checkpoint.h; the reference's SaveModel and USE_OLD_MODEL,
// tests/src/LRServer.h:107-115, 36-63):
//   opt   KVServerRowOptHandle(W, lr, Adam)    one worker
//   sync  KVServerRowSyncHandle(W, lr, Adam)   every worker's Push in each round
//   acc   KVServerRowHandle<float>(W)          accumulate only, no iteration
// Every worker builds the same list of distinct keys spread over the whole key
// range.  Worker 0 seeds every row (cmd = 2 for opt / sync).  Iteration `it` is
// one gradient Push per worker on an ascending list of its own — about half of
// the keys, always the lowest and the highest — worker 0's with cmd = 1, which
// ends the iteration on every server.  Seeds and gradients are functions of
// (iteration, worker, key, column) alone, so two jobs send the same values.
//
//   phase save:    seed, iterations 0-1;                              barrier
//                  every server SaveModel(dir/shard-<rank>);          barrier
//                  worker 0 pulls every row into dir/mid; iterations 2-3;
//                  worker 0 pulls every row into dir/final.
//   phase resume:  every server LoadModel(dir/shard-<r>) for r < saved_ns and
//                  checks iteration() == 2 (opt / sync) and that the rows it
//                  loaded are the keys of its own range;              barrier
//                  every worker's Pull equals dir/mid; iterations 2-3; every
//                  worker's Pull equals dir/final.
//   phase badwidth: a server whose handle has width W + 1 loads dir/shard-0:
//                  the CHECK fails and its table stays empty.
// A two-frame f32 sum from zero does not depend on arrival order, so the sync
// job with two workers is deterministic.  Exits non-zero on the first mismatch.
// usage: kv_rows_ckpt_device [-ns S] [-nw W] [-procs] handle width num_keys dir phase saved_ns
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "internal/device.h"
#include "ps/ps.h"

using namespace ps;

static constexpr float kLr = 0.01f;
static constexpr int kAllButScheduler = kServerGroup + kWorkerGroup;

// a float in [-1, 1) from (a, b, key, column): splitmix64 of their mix
static float Value(uint64_t a, uint64_t b, Key key, uint64_t col) {
  uint64_t z = key + 0x9e3779b97f4a7c15ull * (a * 1315423911ull + b * 2654435761ull + col + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (float)(z >> 40) / 8388608.0f - 1.0f;
}

static std::vector<float> Values(uint64_t a, uint64_t b, const std::vector<Key>& keys, size_t w) {
  std::vector<float> v(keys.size() * w);
  for (size_t i = 0; i < keys.size(); ++i)
    for (size_t j = 0; j < w; ++j) v[i * w + j] = Value(a, b, keys[i], j);
  return v;
}

static void WriteFile(const std::string& path, const std::vector<float>& v) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  f.write((const char*)v.data(), v.size() * sizeof(float));
  CHECK(f.good()) << "writing " << path;
}

static void CompareFile(const std::string& path, const std::vector<float>& got) {
  std::ifstream f(path, std::ios::binary);
  CHECK(f.is_open()) << path << " is missing";
  std::vector<float> exp(got.size());
  f.read((char*)exp.data(), exp.size() * sizeof(float));
  CHECK_EQ((size_t)f.gcount(), exp.size() * sizeof(float)) << path << " is too short";
  CHECK(f.peek() == EOF) << path << " is too long";
  for (size_t i = 0; i < got.size(); ++i) {
    uint32_t a, b;
    std::memcpy(&a, &got[i], 4);
    std::memcpy(&b, &exp[i], 4);
    CHECK_EQ(a, b) << path << ", value " << i << ": pulled " << got[i] << ", the uninterrupted job " << exp[i];
  }
}

static uint64_t TableSize(psg_table* t) {
  if (!t) return 0;
  psg_table_info info;
  device::Check(psg_table_get_info(t, &info), "psg_table_get_info");
  return info.size;
}

// the server's side of a phase, on the node's main thread, for one handle type
template <typename Handle, typename Server>
static void ServerPhase(Handle handle, Server* server, const std::string& dir, const std::string& phase, int saved_ns,
                        bool counts) {
  server->SetDeviceRequestHandle(handle);  // a copy: it shares the handle's state
  RegisterExitCallback([server]() { delete server; });
  const std::string mine = dir + "/shard-" + std::to_string(MyRank());
  if (phase == "save") {
    Barrier(0, kAllButScheduler);  // iterations 0-1 are applied and answered
    handle.SaveModel(mine);
    Barrier(0, kAllButScheduler);
  } else if (phase == "resume") {
    int loaded = 0;
    for (int r = 0; r < saved_ns; ++r) loaded += handle.LoadModel(dir + "/shard-" + std::to_string(r));
    CHECK_EQ((uint64_t)loaded, TableSize(handle.state->table)) << "every loaded key is a row of its own";
    if constexpr (requires { handle.iteration(); }) {
      if (counts) CHECK_EQ(handle.iteration(), 2) << "LoadModel sets the iteration to the file's";
    }
    Barrier(0, kAllButScheduler);
  } else {
    bool failed = false;
    try {
      handle.LoadModel(dir + "/shard-0");
    } catch (const ps_log::PSError& e) {
      failed = std::strstr(e.what(), "width") != nullptr;
    }
    CHECK(failed) << "a file of another width was loaded";
    CHECK_EQ(TableSize(handle.state->table), (uint64_t)0) << "a refused load wrote rows";
    std::printf("rows ckpt badwidth ok\n");
    std::fflush(stdout);
  }
}

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  CHECK(argc > 9) << "usage: kv_rows_ckpt_device handle width num_keys dir phase saved_ns";
  const std::string kind = argv[4];
  const size_t w = (size_t)std::atol(argv[5]);
  const size_t n = (size_t)std::atol(argv[6]);
  const std::string dir = argv[7];
  const std::string phase = argv[8];
  const int saved_ns = std::atoi(argv[9]);
  const bool bad = phase == "badwidth";
  CHECK(kind == "opt" || kind == "sync" || kind == "acc") << kind;
  CHECK(phase == "save" || phase == "resume" || bad) << phase;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    const uint32_t hw = (uint32_t)(bad ? w + 1 : w);
    if (kind == "opt")
      ServerPhase(KVServerRowOptHandle(hw, kLr, true), server, dir, phase, saved_ns, true);
    else if (kind == "sync")
      ServerPhase(KVServerRowSyncHandle(hw, kLr, true), server, dir, phase, saved_ns, true);
    else
      ServerPhase(KVServerRowHandle<float>(hw), server, dir, phase, saved_ns, false);
  }
  if (IsWorker() && !bad) {
    const int rank = MyRank();
    const int dev = PostOffice::Get()->device();
    KVWorker<float> kv(0, 0);
    auto to_dev = [&](const auto& v) {
      using T = typename std::decay_t<decltype(v)>::value_type;
      auto d = SVector<T>::OnDevice(v.size(), dev);
      device::CopySync(d.data(), v.data(), v.size() * sizeof(T), 0);
      return d;
    };
    std::mt19937_64 shared(99);
    std::vector<Key> all;
    while (all.size() < n) {
      for (size_t i = all.size(); i < n; ++i) all.push_back(shared() % kMaxKey);
      std::sort(all.begin(), all.end());
      all.erase(std::unique(all.begin(), all.end()), all.end());
    }
    const int seed_cmd = kind == "acc" ? 0 : 2;  // kAccumulate of the two training handles
    auto train = [&](int it) {
      std::mt19937_64 rng(1000 * (it + 1) + rank);
      std::vector<Key> sub;
      for (size_t i = 0; i < all.size(); ++i)
        if (i == 0 || i + 1 == all.size() || (rng() & 1)) sub.push_back(all[i]);
      const int cmd = kind == "acc" ? 0 : rank == 0 ? 1 : 0;
      kv.Wait(kv.ZPush(to_dev(sub), to_dev(Values(it + 1, rank, sub, w)), {}, cmd));
      Barrier(0, kWorkerGroup);
    };
    auto pull_all = [&]() {
      std::vector<float> out;
      kv.Wait(kv.Pull(all, &out));
      CHECK_EQ(out.size(), all.size() * w);
      return out;
    };
    if (phase == "save") {
      if (rank == 0) kv.Wait(kv.ZPush(to_dev(all), to_dev(Values(0, 0, all, w)), {}, seed_cmd));
      Barrier(0, kWorkerGroup);
      train(0);
      train(1);
      Barrier(0, kAllButScheduler);
      Barrier(0, kAllButScheduler);  // the shards are written
      if (rank == 0) WriteFile(dir + "/mid", pull_all());
      Barrier(0, kWorkerGroup);
      train(2);
      train(3);
      if (rank == 0) WriteFile(dir + "/final", pull_all());
    } else {
      Barrier(0, kAllButScheduler);  // the shards are loaded
      CompareFile(dir + "/mid", pull_all());
      Barrier(0, kWorkerGroup);
      train(2);
      train(3);
      CompareFile(dir + "/final", pull_all());
    }
    std::printf("rows ckpt %s ok: worker %d of %d, %s, width %zu, %zu keys\n", phase.c_str(), rank, NumWorkers(),
                kind.c_str(), w, all.size());
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
