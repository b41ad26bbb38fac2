// kv_rows_any_device.cpp — key lists with repeats, and in any order, on rows of
// W floats per key, end to end through KVWorker / KVServer on the GPU data path
// (run by tests/test_rows_any_dropin_gpu.py).
//
// mode 0: the servers run KVServerRowHandle<float>(W, true) (ps/row_handle.h
//   with any_order: psg_table_handle_any on a psg_table in HBM).
// mode 1: the servers run KVServerRowOptHandle(W, lr, false, 0, true)
//   (ps/row_opt_handle.h with any_order: SGD by psg_table_update_any; the seed
//   is a cmd = 2 accumulate Push).
//
// Every worker sends, on keys of its own (key % nw == rank):
//   ZPush / ZPushPull / ZPull of a non-descending list with repeats as HBM
//     frames (sliced per server by lower_bound: all repeats of a key land on
//     one server),
//   Push / PushPull / Pull of another such list as host vectors, mixing the
//     first list's keys with new ones (the table inserts each once),
//   and at one server and one worker — where the slicer passes an HBM list on
//     whole — a shuffled HBM list with repeats.
// Each request is replayed on a host map with the reference's loop
// (src/ps/KVApp.h:446-454; for mode 1 the update of tests/src/LRServer.h:182-189)
// per occurrence in arrival order, and every pulled value is compared bit for
// bit.  The harness rule of the Makefile compiles this file with
// -ffp-contract=off.  Exits non-zero on the first mismatch.
// usage: kv_rows_any_device [-ns S] [-nw W] [-procs] [width] [num_occurrences] [mode]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <random>
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
  const bool opt = argc > 6 ? std::atol(argv[6]) != 0 : false;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    if (opt)
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
    std::mt19937_64 rng(4321 + rank);
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
    // `count` occurrences drawn from `from` (each key about count / from.size()
    // times, some of them never), non-descending
    auto occurrences = [&](size_t count, const std::vector<Key>& from) {
      std::vector<Key> k(count);
      for (auto& x : k) x = from[rng() % from.size()];
      std::sort(k.begin(), k.end());
      return k;
    };
    auto values = [&](size_t count) {
      std::vector<float> v(count * w);
      for (auto& x : v) x = (float)((double)(rng() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };
    // the Push of this mode: a gradient Push (cmd 0) to the optimizer handle
    const int cmd = 0;
    Rows ref;

    // ---- seed (mode 1): an accumulate Push with repeats ----------------------------
    const std::vector<Key> da = fresh_keys(n / 4 + 1, {});
    if (opt) {
      const std::vector<Key> s = occurrences(n, da);
      const std::vector<float> vs = values(s.size());
      kv.Wait(kv.ZPush(to_dev(s), to_dev(vs), {}, KVServerRowOptHandle::kAccumulate));
      Replay(ref, w, s, vs, true, false, false);
    }

    // ---- HBM frames: non-descending with repeats -----------------------------------
    const std::vector<Key> a = occurrences(n, da);
    const std::vector<float> va = values(n);
    auto dk = to_dev(a);
    auto dv = to_dev(va);
    kv.Wait(kv.ZPush(dk, dv, {}, cmd));
    Replay(ref, w, a, va, true, false, opt);
    auto dout = SVector<float>::OnDevice(n * w, dev);
    kv.Wait(kv.ZPushPull(dk, dv, &dout, nullptr, cmd));
    Compare(to_host(dout), Replay(ref, w, a, va, true, true, opt), "HBM PushPull with repeats");
    auto dout2 = SVector<float>::OnDevice(n * w, dev);
    kv.Wait(kv.ZPull(dk, &dout2));
    Compare(to_host(dout2), Replay(ref, w, a, va, false, true, opt), "HBM Pull with repeats");

    // ---- host vectors: the first list's keys mixed with new ones -------------------
    std::vector<Key> db;
    for (size_t i = 0; i < da.size(); i += 2) db.push_back(da[i]);
    for (Key k : fresh_keys(n / 8 + 1, da)) db.push_back(k);
    std::sort(db.begin(), db.end());
    const std::vector<Key> b = occurrences(n, db);
    const std::vector<float> vb = values(b.size());
    kv.Wait(kv.Push(b, vb, {}, cmd));
    Replay(ref, w, b, vb, true, false, opt);
    std::vector<float> outs;
    kv.Wait(kv.PushPull(b, vb, &outs, nullptr, cmd));
    Compare(outs, Replay(ref, w, b, vb, true, true, opt), "host PushPull with repeats");
    std::vector<float> pulled;
    kv.Wait(kv.Pull(b, &pulled));
    Compare(pulled, Replay(ref, w, b, vb, false, true, opt), "host Pull with repeats");
    // list a again: rows moved and were pushed to since
    kv.Wait(kv.ZPull(dk, &dout2));
    Compare(to_host(dout2), Replay(ref, w, a, va, false, true, opt), "HBM Pull after the inserts");

    // ---- one server, one worker: a shuffled HBM list with repeats ------------------
    if (NumServers() == 1 && nw == 1) {
      std::vector<Key> dc = db;
      for (Key k : fresh_keys(n / 8 + 1, db)) dc.push_back(k);
      std::vector<Key> c = occurrences(n, dc);
      std::shuffle(c.begin(), c.end(), rng);
      const std::vector<float> vc = values(c.size());
      auto dkc = to_dev(c);
      auto dvc = to_dev(vc);
      kv.Wait(kv.ZPush(dkc, dvc, {}, cmd));
      Replay(ref, w, c, vc, true, false, opt);
      auto doc = SVector<float>::OnDevice(c.size() * w, dev);
      kv.Wait(kv.ZPushPull(dkc, dvc, &doc, nullptr, cmd));
      Compare(to_host(doc), Replay(ref, w, c, vc, true, true, opt), "shuffled HBM PushPull");
      auto doc2 = SVector<float>::OnDevice(c.size() * w, dev);
      kv.Wait(kv.ZPull(dkc, &doc2));
      Compare(to_host(doc2), Replay(ref, w, c, vc, false, true, opt), "shuffled HBM Pull");
    }

    std::printf("rows any ok: worker %d, width %zu, %zu occurrences, %s\n", rank, w, n, opt ? "SGD" : "accumulate");
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
