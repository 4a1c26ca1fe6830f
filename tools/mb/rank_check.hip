// Check of the ring sort's stable rank by bit ballots (dev_common.hpp wave_key_rank) against a
// serial reference on the host: per wave, every valid lane's rank among the valid lanes of its key
// in lower lanes, and that key's count as stored by the lane with rank 0.  Waves hold one key, two
// keys, all R keys (R = 16 and 64, in firing order and at random), invalid lanes interleaved
// (their key is 255, as the ring kernels leave it), and no valid lane at all.  Built by
// loam_velodyne-1_amd/Makefile; run by tests/test_gpu_rank.py.  Exit 0 when every result matches.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>

#include "../../loam_velodyne-1_amd/csrc/dev_common.hpp"

using namespace loamdev;

// out: per lane the rank (-1 for an invalid lane); cnt: per wave 64 counts, as the kernels' sh_wcnt
__global__ void k_rank(const int* key, const int* R, int* out, int* cnt) {
  const int w = blockIdx.x, lane = lane_id();
  __shared__ int sh_cnt[64];
  sh_cnt[lane] = 0;
  __builtin_amdgcn_wave_barrier();
  const int k = key[w * 64 + lane];
  const bool valid = k != 255;
  int peers;
  const int rank = wave_key_rank(k, valid, key_bits(R[w]), peers);
  if (valid && rank == 0) sh_cnt[k] = peers;
  __syncthreads();
  out[w * 64 + lane] = valid ? rank : -1;
  cnt[w * 64 + lane] = sh_cnt[lane];
}

int main() {
  std::mt19937 rng(11);
  std::vector<int> key, R;
  auto wave = [&](int r, auto&& f) {
    R.push_back(r);
    for (int l = 0; l < 64; ++l) key.push_back(f(l));
  };
  for (int r : {2, 3, 16, 17, 33, 64}) {
    for (int rep = 0; rep < 16; ++rep) {
      const int a = rng() % r, b = rng() % r;
      wave(r, [&](int) { return a; });                                  // one key
      wave(r, [&](int) { return rng() & 1 ? a : b; });                  // two keys
      wave(r, [&](int l) { return (l + rep) % r; });                    // all keys, firing order
      wave(r, [&](int) { return (int)(rng() % r); });                   // all keys, random
      wave(r, [&](int l) { return (l + rep) % 3 == 0 ? 255 : (int)(rng() % r); });  // invalid lanes interleaved
      wave(r, [&](int l) { return rng() % 4 ? 255 : r - 1; });          // mostly invalid, the top key (63: 255's low bits)
      wave(r, [&](int) { return 255; });                                // all lanes invalid
      wave(r, [&](int l) { return l == (int)(rep * 4 + 1) ? r - 1 : 255; });  // one valid lane
    }
  }
  const int W = (int)R.size();
  int *dk, *dr, *dout, *dcnt;
  (void)hipMalloc(&dk, key.size() * 4);
  (void)hipMalloc(&dr, R.size() * 4);
  (void)hipMalloc(&dout, key.size() * 4);
  (void)hipMalloc(&dcnt, key.size() * 4);
  (void)hipMemcpy(dk, key.data(), key.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dr, R.data(), R.size() * 4, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_rank, dim3(W), dim3(64), 0, 0, dk, dr, dout, dcnt);
  std::vector<int> out(key.size()), cnt(key.size());
  if (hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(cnt.data(), dcnt, cnt.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    std::printf("hip error\n");
    return 2;
  }
  int bad = 0;
  for (int w = 0; w < W; ++w) {
    int seen[256] = {0};
    for (int l = 0; l < 64; ++l) {
      const int k = key[w * 64 + l];
      const int want = k == 255 ? -1 : seen[k]++;
      if (out[w * 64 + l] != want && bad++ < 10)
        std::printf("wave %d (R %d) lane %d key %d: rank %d, want %d\n", w, R[w], l, k, out[w * 64 + l], want);
    }
    for (int k = 0; k < 64; ++k)
      if (cnt[w * 64 + k] != seen[k] && bad++ < 10)
        std::printf("wave %d (R %d) key %d: count %d, want %d\n", w, R[w], k, cnt[w * 64 + k], seen[k]);
  }
  std::printf("rank_check: %d waves, %d mismatches\n", W, bad);
  return bad ? 1 : 0;
}
