// The tile-parallel form of scanRegistration's forward-only IMU queue walk (sr.hip
// k_sr_ring_count<true> / k_sr_ring_scatter<true>), run on the host from the shared
// pieces of loam_velodyne-1_amd/csrc/imu.hpp (ori_first / ori_second, the orientation keys,
// tile_ori_key, first_later_of) against the sequential walk of k_sr_ring_sort<true>: every
// ring-filtered point's queue entry and the pointer the sweep leaves.
// The sweeps are adversarial, not physical: orientations that mostly advance but jitter and jump
// backwards and forwards by whole fractions of a turn, flips anywhere (a tile with a flip of its own
// behind the sweep's flip, no flip at all), dropped points in runs longer than a tile, tiles of 1 to
// 64 points, queues that wrap, queues whose stamps all precede or all follow the sweep.
// Then the host / device hand-off of the queue entries (lane_records, lane_record_put): messages
// pushed in bursts of 0 to 450 between steps, each step's records applied to a mirror queue, which
// must hold the host queue's entries wherever the last 200 messages lie.
// Prints "<sweeps> <points checked> <mismatches> <queue steps checked>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/imu.hpp"

namespace {

using namespace loamimu;

uint64_t g_s = 0x2545f4914f6cdd1dull;
double rnd() {  // [0, 1)
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return (double)(g_s >> 11) / 9007199254740992.0;
}
int rndi(int n) { return (int)(rnd() * n); }

struct Sweep {
  std::vector<float> ori;      // -atan2 of each point
  std::vector<uint8_t> valid;  // passed the ring filter
  float startOri, endOri;
  double time_scan;
};

float point_time(float o, float startOri, float endOri) {
  const float relTime = (o - startOri) / (endOri - startOri);
  return (float)(D(relTime) * 0.1);
}

// k_sr_ring_sort<true>: F over the ring-filtered points, then the walk in input order
void walk_serial(const Sweep& s, const SrQueue& q, std::vector<int>& front, int& F, int& left) {
  const int n = (int)s.ori.size();
  F = 0x7fffffff;
  for (int i = 0; i < n; ++i)
    if (s.valid[i] && D(ori_first(s.ori[i], s.startOri) - s.startOri) > M_PI) { F = i; break; }
  int carry = 0;
  front.assign(n, -1);
  for (int i = 0; i < n; ++i) {
    if (!s.valid[i]) continue;
    const float o = i <= F ? ori_first(s.ori[i], s.startOri) : ori_second(s.ori[i], s.endOri);
    const int g = first_later(q, q.front, s.time_scan + point_time(o, s.startOri, s.endOri));
    carry = carry > g ? carry : g;
    front[i] = carry;
  }
  left = (q.front + carry) % kQue;
}

// the count pass (per-tile first flip and the three keys), then every tile on its own
void walk_tiled(const Sweep& s, const SrQueue& q, int tile, std::vector<int>& front, int& F, int& left, bool& wrote) {
  const int n = (int)s.ori.size(), nt = (n + tile - 1) / tile;
  std::vector<int> key(3 * nt, kNoOri), tileF(nt, 0x7fffffff);
  for (int t = 0; t < nt; ++t) {
    const int a = t * tile, b = a + tile < n ? a + tile : n;
    for (int i = a; i < b; ++i)
      if (s.valid[i] && D(ori_first(s.ori[i], s.startOri) - s.startOri) > M_PI) { tileF[t] = i; break; }
    for (int i = a; i < b; ++i) {
      if (!s.valid[i]) continue;
      const int k1 = ori_key(ori_first(s.ori[i], s.startOri)), k2 = ori_key(ori_second(s.ori[i], s.endOri));
      int* k = &key[3 * t];
      if (i <= tileF[t]) { k[0] = k[0] > k1 ? k[0] : k1; k[2] = k[2] > k2 ? k[2] : k2; }
      else k[1] = k[1] > k2 ? k[1] : k2;
    }
  }
  F = 0x7fffffff;
  for (int t = 0; t < nt; ++t) F = F < tileF[t] ? F : tileF[t];
  const int tF = F == 0x7fffffff ? 0x7fffffff : F / tile;
  front.assign(n, -1);
  wrote = false;
  left = q.front;
  for (int t = nt - 1; t >= 0; --t) {  // (any order: the tiles do not depend on each other)
    int carry = 0;
    for (int u = 0; u < t; ++u) {
      const int k = tile_ori_key(&key[3 * u], u, tF);
      if (k == kNoOri) continue;
      const int g = first_later_of(q.time, q.last, q.front, s.time_scan + point_time(ori_of_key(k), s.startOri, s.endOri));
      carry = carry > g ? carry : g;
    }
    const int a = t * tile, b = a + tile < n ? a + tile : n;
    int last = -1;
    for (int i = a; i < b; ++i) {
      if (!s.valid[i]) continue;
      const float o = i <= F ? ori_first(s.ori[i], s.startOri) : ori_second(s.ori[i], s.endOri);
      const int g = first_later_of(q.time, q.last, q.front, s.time_scan + point_time(o, s.startOri, s.endOri));
      carry = carry > g ? carry : g;
      front[i] = carry;
      last = i;
    }
    bool later = false;  // a later tile has a ring-filtered point
    for (int i = b; i < n && !later; ++i) later = s.valid[i] != 0;
    if (last >= 0 && !later) {
      left = (q.front + front[last]) % kQue;
      wrote = true;
    }
  }
}

Sweep make_sweep(int n, double time_scan) {
  Sweep s;
  s.time_scan = time_scan;
  s.ori.resize(n);
  s.valid.resize(n);
  const float a0 = (float)((rnd() * 2 - 1) * M_PI);
  const double turn = 2 * M_PI * (0.85 + 0.3 * rnd());
  const int mode = rndi(4);
  int drop_from = -1, drop_to = -1;
  if (rndi(3) == 0) { drop_from = rndi(n); drop_to = drop_from + rndi(n); }
  for (int i = 0; i < n; ++i) {
    double a = a0 + turn * i / n + (rnd() - 0.5) * 0.02;
    if (mode >= 1 && rndi(40) == 0) a += (rnd() - 0.5) * 2.0;       // jumps of up to a sixth of a turn
    if (mode == 2 && rndi(200) == 0) a += (rnd() - 0.5) * 2 * M_PI;  // and of up to half a turn
    if (mode == 3) a = a0 + turn * 0.4 * i / n;                       // never reaches the flip
    a = std::fmod(a + M_PI, 2 * M_PI);
    if (a < 0) a += 2 * M_PI;
    s.ori[i] = (float)(a - M_PI);  // as -atan2 gives it: [-pi, pi)
    s.valid[i] = rndi(10) != 0 && !(i >= drop_from && i < drop_to);
  }
  // :230-238 from the first / last point (finite, whether or not they pass the ring filter)
  s.startOri = s.ori[0];
  s.endOri = (float)(D(s.ori[n - 1]) + 2 * M_PI);
  if (D(s.endOri - s.startOri) > 3 * M_PI) s.endOri = (float)(D(s.endOri) - 2 * M_PI);
  else if (D(s.endOri - s.startOri) < M_PI) s.endOri = (float)(D(s.endOri) + 2 * M_PI);
  return s;
}

SrQueue make_queue(double time_scan) {
  SrQueue q{};
  const int count = 1 + rndi(kQue - 1);  // entries between front and last, no lap
  q.front = rndi(kQue);
  q.last = (q.front + count - 1) % kQue;
  const int where = rndi(5);  // 0: all before the sweep, 1: all after, else around it
  double t = where == 0 ? time_scan - 1.0 : where == 1 ? time_scan + 0.2 : time_scan - 0.05 * rnd();
  const double step = where == 0 ? 0.9 / count : (0.0005 + 0.02 * rnd());
  for (int k = 0; k < count; ++k) {
    q.time[(q.front + k) % kQue] = t;
    if (rndi(8) != 0) t += step * rnd() * 2;  // (equal stamps now and then)
  }
  return q;
}

// bursts of messages between steps; returns the mismatches
long check_records(long& steps) {
  long bad = 0;
  for (int rep = 0; rep < 200; ++rep) {
    SrQueue host{}, mirror{};
    host.last = mirror.last = -1;
    std::vector<LaneRec> rec(kQue);
    double t = 10.0 * rnd();
    long total = 0;
    for (int step = 0; step < 12; ++step) {
      const int burst = rndi(6) == 0 ? 200 + rndi(251) : rndi(60);
      for (int k = 0; k < burst; ++k) {
        t += 0.01 * rnd();
        const double acc[3] = {rnd(), rnd(), 9.81 + rnd()};
        sr_push(host, t, 0.01 * rnd(), 0.01 * rnd(), rnd(), acc);
      }
      total += burst;
      const int m = lane_records(host, burst, 7, rec.data());
      if (m != (burst < kQue ? burst : kQue)) ++bad;
      for (int j = 0; j < m; ++j) {
        if (rec[j].lane != 7 || rec[j].idx < 0 || rec[j].idx >= kQue) { ++bad; continue; }
        lane_record_put(mirror, rec[j]);
      }
      if (m > 0 && rec[m - 1].idx != host.last) ++bad;
      mirror.last = host.last;
      // every entry a reader may touch: the last min(total, kQue) messages
      const long live = total < kQue ? total : kQue;
      for (long j = 0; j < live; ++j) {
        const int k = (int)(((host.last - j) % kQue + kQue) % kQue);
        if (mirror.time[k] != host.time[k] || mirror.roll[k] != host.roll[k] || mirror.yaw[k] != host.yaw[k] ||
            mirror.accZ[k] != host.accZ[k] || mirror.veloX[k] != host.veloX[k] || mirror.shiftZ[k] != host.shiftZ[k] ||
            mirror.pitch[k] != host.pitch[k] || mirror.shiftX[k] != host.shiftX[k])
          ++bad;
      }
      ++steps;
    }
  }
  return bad;
}

}  // namespace

int main() {
  long sweeps = 0, checked = 0, bad = 0;
  const int tiles[] = {1, 2, 3, 7, 16, 64};
  for (int rep = 0; rep < 4000; ++rep) {
    const int n = 1 + rndi(400);
    const double time_scan = rndi(2) ? 0.1 * rndi(1000) : 1.7e9 + 0.1 * rndi(1000);
    const Sweep s = make_sweep(n, time_scan);
    const SrQueue q = make_queue(time_scan);
    std::vector<int> fa, fb;
    int Fa, Fb, la, lb;
    walk_serial(s, q, fa, Fa, la);
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || s.valid[i];
    for (int tile : tiles) {
      bool wrote;
      walk_tiled(s, q, tile, fb, Fb, lb, wrote);
      ++sweeps;
      if (Fa != Fb || la != lb || wrote != any) ++bad;
      for (int i = 0; i < n; ++i) {
        if (!s.valid[i]) continue;
        ++checked;
        if (fa[i] != fb[i]) ++bad;
      }
    }
  }
  long steps = 0;
  bad += check_records(steps);
  std::printf("%ld %ld %ld %ld\n", sweeps, checked, bad, steps);
  return bad ? 1 : 0;
}
