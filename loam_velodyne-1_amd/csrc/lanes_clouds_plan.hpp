// loam_lanes_clouds' chunk planning (host only, no HIP: tests/lanes_clouds_plan_check.cpp drives it).
// The packed selection leaves the device through a fixed staging; a chunk is a run of consecutive
// list entries whose wanted clouds fit one staging buffer together.
#ifndef LOAM_LANES_CLOUDS_PLAN_HPP
#define LOAM_LANES_CLOUDS_PLAN_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace loam {

constexpr int kLaneClouds = 9;  // LOAM_LANE_CLOUDS, in loam_lanes_clouds_out's order

// entries [j0, j1) of the list; cloud c's points of the chunk lie in the staging at [cbase[c],
// cbase[c] + T[c][j1] - T[c][j0]) and are points [T[c][j0], T[c][j1]) of the cloud's selection
struct LaneCloudsChunk {
  uint32_t j0, j1;
  uint64_t cbase[kLaneClouds];
  uint64_t pts;  // of all wanted clouds: <= the staging
};

// T: the offsets table [kLaneClouds][n + 1] (row c: exclusive prefix sums of cloud c's counts over the
// list, T[c][n] the total); clouds: bit c = cloud c's points are wanted; stage: points of one staging
// buffer.  Fills `chunks` (entries in order, every entry with points in exactly one chunk, chunks
// without points left out) and returns true; false with *bad = the entry whose wanted clouds alone
// exceed the staging (chunks is then empty).
inline bool lanes_clouds_plan(const uint64_t* T, uint32_t n, unsigned clouds, uint64_t stage,
                              std::vector<LaneCloudsChunk>& chunks, uint32_t* bad) {
  chunks.clear();
  const size_t row = (size_t)n + 1;
  auto span = [&](uint32_t a, uint32_t b) {
    uint64_t s = 0;
    for (int c = 0; c < kLaneClouds; ++c)
      if (clouds >> c & 1) s += T[c * row + b] - T[c * row + a];
    return s;
  };
  for (uint32_t j0 = 0; j0 < n;) {
    if (span(j0, j0 + 1) > stage) {
      chunks.clear();
      *bad = j0;
      return false;
    }
    uint32_t j1 = j0 + 1;
    while (j1 < n && span(j0, j1 + 1) <= stage) ++j1;
    LaneCloudsChunk ch;
    ch.j0 = j0;
    ch.j1 = j1;
    ch.pts = 0;
    for (int c = 0; c < kLaneClouds; ++c) {
      ch.cbase[c] = ch.pts;
      if (clouds >> c & 1) ch.pts += T[c * row + j1] - T[c * row + j0];
    }
    if (ch.pts) chunks.push_back(ch);
    j0 = j1;
  }
  return true;
}

}  // namespace loam
#endif
