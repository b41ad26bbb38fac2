// kv_rows_adagrad_device.cpp — rows trained with row-wise Adagrad in sync-mode
// rounds, end to end through KVWorker / KVServer on the GPU data path (run by
// tests/test_rows_adagrad_dropin_gpu.py).
//
// The servers run KVServerRowSyncHandle(W, lr, false) with SetAdagrad(eps, init)
// (ps/row_sync_handle.h: one psg_table_update_merged per round, which steps an
// Adagrad table with k_rows_walk_rowwise).  For rounds 0, 1, 2 every worker
// Pushes gradients with ZPushAny on a list in no order and with repeats, spread
// over the whole key range, worker 0 with cmd = 1; then worker 0 Pulls every key
// with ZPullAny and prints each row as hex words.  Nothing is checked here: the
// pytest replays the rounds on ONE whole-range model and compares bit for bit.
// Keys and gradients are the formulas below, which the pytest restates.  The
// gradients are small integers, so a key's f32 sum does not depend on the order
// in which the servers see the workers' Pushes.
// usage: kv_rows_adagrad_device [-ns S] [-nw W] [width]
#include <cstdio>
#include <cstring>
#include <vector>

#include "internal/device.h"
#include "ps/ps.h"

using namespace ps;

static constexpr float kLr = 0.05f;
static constexpr double kEps = 1e-8, kInit = 0.125;
static constexpr int kRounds = 3, kIds = 50, kOccurrences = 80;
static constexpr Key kStride = kMaxKey / 64;  // id j is key j * kStride + 1: both servers own some

static Key KeyOf(int rank, int round, int i) { return (Key)((i * 7 + rank * 3 + round * 11) % kIds) * kStride + 1; }
static float GradOf(int rank, int round, int i, int c) { return (float)((i + 2 * c + rank + round) % 7 - 3); }

int main(int argc, char* argv[]) {
  Start(0, argc, argv);
  const size_t w = argc > 3 ? (size_t)std::atol(argv[argc - 1]) : 8;
  if (IsServer()) {
    auto server = new KVServer<float>(0);
    KVServerRowSyncHandle handle((uint32_t)w, kLr, false);
    handle.SetAdagrad(kEps, kInit);
    server->SetDeviceRequestHandle(handle);
    RegisterExitCallback([server]() { delete server; });
  }
  if (IsWorker()) {
    const int rank = MyRank();
    const int dev = PostOffice::Get()->device();
    KVWorker<float> kv(0, 0);
    auto to_dev = [&](const auto& v) {
      using T = typename std::decay_t<decltype(v)>::value_type;
      auto d = SVector<T>::OnDevice(v.size(), dev);
      device::CopySync(d.data(), v.data(), v.size() * sizeof(T), 0);
      return d;
    };
    for (int round = 0; round < kRounds; ++round) {
      std::vector<Key> keys(kOccurrences);
      std::vector<float> grads(kOccurrences * w);
      for (int i = 0; i < kOccurrences; ++i) {
        keys[i] = KeyOf(rank, round, i);
        for (size_t c = 0; c < w; ++c) grads[i * w + c] = GradOf(rank, round, i, (int)c);
      }
      kv.Wait(kv.ZPushAny(to_dev(keys), to_dev(grads), rank == 0 ? 1 : 0));
      Barrier(0, kWorkerGroup);
    }
    if (rank == 0) {
      std::vector<Key> all(kIds);
      for (int j = 0; j < kIds; ++j) all[j] = (Key)((j * 13) % kIds) * kStride + 1;  // every id, shuffled
      auto out = SVector<float>::OnDevice(kIds * w, dev);
      kv.Wait(kv.ZPullAny(to_dev(all), &out));
      std::vector<float> rows(kIds * w);
      device::CopySync(rows.data(), out.data(), rows.size() * sizeof(float), 1);
      for (int j = 0; j < kIds; ++j) {
        std::printf("row %llu", (unsigned long long)all[j]);
        for (size_t c = 0; c < w; ++c) {
          uint32_t bits;
          std::memcpy(&bits, &rows[j * w + c], 4);
          std::printf(" %08x", bits);
        }
        std::printf("\n");
      }
      std::fflush(stdout);
    }
    Barrier(0, kWorkerGroup);
  }
  Finalize(0, true);
  return 0;
}
