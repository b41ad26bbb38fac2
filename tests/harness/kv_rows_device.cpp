// kv_rows_device.cpp — rows of W values per key end to end through KVWorker /
// KVServer on the GPU data path (run by tests/test_rows_dropin_gpu.py).
//
// The servers run KVServerRowHandle<float>(W) (ps/row_handle.h: a psg_table
// in HBM).  Every worker sends requests whose values hold W floats per key —
// the k = vals.size() / keys.size() contract of the reference's DefaultSlicer
// (src/ps/KVApp.h:515-574), which cuts keys and values per server, and of its
// pull merge (KVApp.h:673-726):
//   ZPush / ZPushPull / ZPull on HBM SVectors (frames read in place, a Pull's
//     reply written into the worker's output slice),
//   Push / PushPull / Pull on host vectors (staged by the server, replies
//     merged on the host), on a list that interleaves the first one's keys
//     with new ones (the table inserts and moves rows),
//   a ZPull of keys never pushed (zero rows).
// Each request is replayed on a std::unordered_map<Key, std::vector<float>>
// with the reference's loop (KVApp.h:446-454) per element, and every pulled
// value is compared bit for bit.  Workers use disjoint keys (key % nw == rank),
// so each one's replay is exact whatever the others do.  Exits non-zero on the
// first mismatch.
// usage: kv_rows_device [-ns S] [-nw W] [-procs] [width] [num_keys]
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

static std::vector<float> Replay(Rows& table, size_t w, const std::vector<Key>& keys, const std::vector<float>& vals,
                                 bool push, bool pull) {
  std::vector<float> out(pull ? keys.size() * w : 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    std::vector<float>& row = table[keys[i]];
    if (row.empty()) row.assign(w, 0.0f);
    for (size_t j = 0; j < w; ++j) {
      if (push) row[j] += vals[i * w + j];
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
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    server->SetDeviceRequestHandle(KVServerRowHandle<float>((uint32_t)w));
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const Key nw = (Key)NumWorkers();
    const int dev = PostOffice::Get()->device();
    KVWorker<float> kv(0, 0);
    std::mt19937_64 rng(1234 + rank);
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
    auto values = [&](size_t count) {
      std::vector<float> v(count * w);
      for (auto& x : v) x = (float)((double)(rng() >> 11) * 0x1p-53 * 2.0 - 1.0);
      return v;
    };
    Rows ref;

    // ---- HBM frames ---------------------------------------------------------------
    const std::vector<Key> a = fresh_keys(n, {});
    const std::vector<float> va = values(n);
    auto dk = to_dev(a);
    auto dv = to_dev(va);
    kv.Wait(kv.ZPush(dk, dv));
    Replay(ref, w, a, va, true, false);
    auto dout = SVector<float>::OnDevice(n * w, dev);
    kv.Wait(kv.ZPushPull(dk, dv, &dout));
    Compare(to_host(dout), Replay(ref, w, a, va, true, true), "HBM PushPull");
    auto dout2 = SVector<float>::OnDevice(n * w, dev);
    kv.Wait(kv.ZPull(dk, &dout2));
    Compare(to_host(dout2), Replay(ref, w, a, va, false, true), "HBM Pull");

    // ---- host vectors, on a list interleaving list a's keys with new ones --------
    std::vector<Key> b;
    for (size_t i = 0; i < a.size(); i += 2) b.push_back(a[i]);
    for (Key k : fresh_keys(n / 2 + 1, a)) b.push_back(k);
    std::sort(b.begin(), b.end());
    const std::vector<float> vb = values(b.size());
    kv.Wait(kv.Push(b, vb));
    Replay(ref, w, b, vb, true, false);
    std::vector<float> outs;
    kv.Wait(kv.PushPull(b, vb, &outs));
    Compare(outs, Replay(ref, w, b, vb, true, true), "host PushPull");
    std::vector<float> pulled;
    kv.Wait(kv.Pull(b, &pulled));
    Compare(pulled, Replay(ref, w, b, vb, false, true), "host Pull");
    // list a again: half of its rows moved and were pushed to since
    kv.Wait(kv.ZPull(dk, &dout2));
    Compare(to_host(dout2), Replay(ref, w, a, va, false, true), "HBM Pull after the inserts");

    // ---- keys never pushed: zero rows ----------------------------------------------
    std::vector<Key> seen = a;
    seen.insert(seen.end(), b.begin(), b.end());
    std::sort(seen.begin(), seen.end());
    const std::vector<Key> c = fresh_keys(n / 3 + 1, seen);
    auto dc = to_dev(c);
    auto dout3 = SVector<float>::OnDevice(c.size() * w, dev);
    kv.Wait(kv.ZPull(dc, &dout3));
    Compare(to_host(dout3), Replay(ref, w, c, {}, false, true), "HBM Pull of absent keys");

    std::printf("rows ok: worker %d, width %zu, %zu keys\n", rank, w, n);
    std::fflush(stdout);
  }
  Finalize(0, true);
  return 0;
}
