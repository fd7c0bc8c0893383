// Context figure of tools/bench_ingest.py --live: what mals_ids_resolve does, on one CPU thread with std::unordered_map -- a
// directory of n_dir ids, then `batches` batches of n_batch ids of which a fraction is new, every id looked up and an
// unknown one given the next row.  usage: ids_map_baseline <n_dir> <n_batch> <new_permille> <batches>; prints ids/s.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int64_t n_dir = std::atoll(argv[1]), n_batch = std::atoll(argv[2]), permille = std::atoll(argv[3]), batches = std::atoll(argv[4]);
  std::unordered_map<int64_t, int64_t> dir;
  dir.reserve((size_t)(n_dir + batches * n_batch));
  for (int64_t r = 0; r < n_dir; ++r) dir.emplace((int64_t)mix((uint64_t)r), r);
  std::vector<int64_t> ids((size_t)n_batch), rows((size_t)n_batch);
  double best = 0.0;
  int64_t next_new = n_dir;
  for (int64_t b = 0; b < batches; ++b) {
    for (int64_t t = 0; t < n_batch; ++t) {
      const uint64_t h = mix((uint64_t)(b * n_batch + t) ^ 0x5555ull);
      ids[(size_t)t] = (int64_t)(h % 1000) < permille ? (int64_t)mix((uint64_t)next_new++) : (int64_t)mix(h % (uint64_t)n_dir);
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t t = 0; t < n_batch; ++t) {
      auto it = dir.find(ids[(size_t)t]);
      if (it == dir.end()) it = dir.emplace(ids[(size_t)t], (int64_t)dir.size()).first;
      rows[(size_t)t] = it->second;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if ((double)n_batch / s > best) best = (double)n_batch / s;
  }
  std::printf("%.0f %lld\n", best, (long long)rows[(size_t)n_batch - 1]);
  return 0;
}
