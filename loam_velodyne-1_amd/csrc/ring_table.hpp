// Ring models as data (LOAM_RING_TABLE): the lookup, the check of a caller's table,
// the two built-in models' ring_id and their restatement as tables.  Host only except for the
// lookup, the built-in rule and the guess polynomial (which the kernels of sr.hip share); no HIP
// call, so the header compiles into a stand-alone program (tests/ring_table_check.cpp).
#ifndef LOAM_RING_TABLE_HPP
#define LOAM_RING_TABLE_HPP

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/loam/loam.h"

#ifdef __HIPCC__
#define LOAM_RT_HD __host__ __device__ __forceinline__
#else
#define LOAM_RT_HD inline
#endif

namespace loam {

constexpr int kRingTableMax = LOAM_RING_TABLE_MAX;  // intervals (65 bounds: the linear model's 64 rings)

// The built-in models (LOAM_RING_VLP16: src/scanRegistration.cpp:248-260; LOAM_RING_LINEAR: the
// HDL-64E hint) on the reference's float vertical angle.
LOAM_RT_HD int ring_id_model(int model, int R, float lo, float hi, float angle) {
  if (model == LOAM_RING_LINEAR) {
    const float step = (hi - lo) / (float)(R - 1);
    const float angleID = (angle - lo) / step;
    return (int)(angleID + 0.5f);
  }
  int rounded = (int)((double)angle + ((double)angle < 0.0 ? -0.5 : +0.5));
  return rounded > 0 ? rounded : rounded + (R - 1);
}

// The table rule: ring[i] for the i with bound[i] <= a < bound[i + 1] (compared as floats); -1
// (dropped) below bound[0], at or above bound[n], for a NaN, and where ring[i] is -1.  A binary
// search of at most 7 halvings (n <= 64 needs 6).
LOAM_RT_HD int ring_table_lookup(const float* bound, const int32_t* ring, int n, float a) {
  if (!(a >= bound[0] && a < bound[n])) return -1;
  int lo = 0, hi = n;  // bound[lo] <= a < bound[hi]
  for (int it = 0; it < 7 && hi - lo > 1; ++it) {
    const int mid = (lo + hi) >> 1;
    if (a >= bound[mid]) lo = mid;
    else hi = mid;
  }
  return ring[lo];
}

// ring_of's interval guess (sr.hip): an odd polynomial for atan, in degrees (good to 0.01 degrees
// over +-25, monotonic inside +-45)
LOAM_RT_HD float ring_guess_deg(float t) {
  const float t2 = t * t;
  return t * fmaf(t2, fmaf(t2, fmaf(t2, -1.0f / 7, 0.2f), -1.0f / 3), 1.0f) * 57.2957795f;
}

// ---------------------------------------------------------------- the check
enum {
  kRingTableOk = 0,
  kRingTableNull,    // a null pointer
  kRingTableRings,   // n_rings outside [2, 64]
  kRingTableN,       // n outside [1, LOAM_RING_TABLE_MAX]
  kRingTableBound,   // a bound that is not finite or not inside (-89, 89)
  kRingTableOrder,   // bounds not strictly ascending
  kRingTableNarrow,  // an interval narrower than 1/32 degree
  kRingTableRing,    // a ring outside [-1, n_rings)
  kRingTableEmpty,   // every ring is -1
  kRingTableModel    // (ring_table_of_model) not a built-in model, or one that cannot be tabulated
};
constexpr double kRingTableMinWidth = 1.0 / 32;  // (the tabulator scans at 1/128 degree)

inline int ring_table_check_why(uint32_t n_rings, uint32_t n, const float* bound, const int32_t* ring) {
  if (!bound || !ring) return kRingTableNull;
  if (n_rings < 2 || n_rings > 64) return kRingTableRings;
  if (n < 1 || n > (uint32_t)kRingTableMax) return kRingTableN;
  for (uint32_t i = 0; i <= n; ++i)
    if (!std::isfinite(bound[i]) || !(bound[i] > -89.0f && bound[i] < 89.0f)) return kRingTableBound;
  for (uint32_t i = 0; i < n; ++i)
    if (!(bound[i] < bound[i + 1])) return kRingTableOrder;
  for (uint32_t i = 0; i < n; ++i)
    if (!((double)bound[i + 1] - (double)bound[i] >= kRingTableMinWidth)) return kRingTableNarrow;
  bool any = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (ring[i] < -1 || ring[i] >= (int32_t)n_rings) return kRingTableRing;
    any = any || ring[i] != -1;
  }
  return any ? kRingTableOk : kRingTableEmpty;
}

inline const char* ring_table_why_text(int why) {
  switch (why) {
    case kRingTableOk: return "ok";
    case kRingTableNull: return "null argument";
    case kRingTableRings: return "n_rings must be in [2, 64]";
    case kRingTableN: return "n must be in [1, LOAM_RING_TABLE_MAX]";
    case kRingTableBound: return "every bound must be finite and inside (-89, 89) degrees";
    case kRingTableOrder: return "the bounds must be strictly ascending";
    case kRingTableNarrow: return "every interval must be at least 1/32 degree wide";
    case kRingTableRing: return "every ring must be in [-1, n_rings)";
    case kRingTableEmpty: return "at least one ring must not be -1";
    default: return "the model cannot be stated as a table of at most LOAM_RING_TABLE_MAX intervals";
  }
}

// ---------------------------------------------------------------- tabulating a step function
// Every float angle in (-89, 89) degrees at which f changes: a scan at 1/128 degree, then bisection
// down to neighbouring floats.  Boundary j lies between last_old[j] and first_new[j] (neighbouring
// floats); val[j] is f between boundary j - 1 and boundary j (val[0]: below the first).  false: two
// changes inside one step of the scan.
struct RingSteps {
  std::vector<float> last_old, first_new;
  std::vector<int> val;
};
template <class F>
bool ring_steps_scan(F f, RingSteps& s) {
  constexpr int G = 128;
  s = RingSteps();
  float a = -89.0f;
  int va = f(a);
  s.val.push_back(va);
  for (int i = 1; i <= 178 * G; ++i) {
    const float c = -89.0f + (float)i / G;
    const int vc = f(c);
    if (vc != va) {
      float lo = a, hi = c;
      for (;;) {
        const float mid = lo + (hi - lo) * 0.5f;
        if (!(mid > lo && mid < hi)) break;
        if (f(mid) == va) lo = mid;
        else hi = mid;
      }
      if (f(hi) != vc) return false;
      s.last_old.push_back(lo);
      s.first_new.push_back(hi);
      s.val.push_back(vc);
    }
    a = c;
    va = vc;
  }
  return true;
}
// the inner intervals (1 .. boundaries - 1) from the first to the last whose value is a ring of
// 0 .. R - 1: false when there is none
inline bool ring_steps_valid_span(const RingSteps& s, int R, int& i0, int& i1) {
  const int nbnd = (int)s.first_new.size();
  i0 = i1 = -1;
  for (int i = 1; i <= nbnd - 1; ++i)
    if (s.val[i] >= 0 && s.val[i] <= R - 1) {
      if (i0 < 0) i0 = i;
      i1 = i;
    }
  return i0 >= 0;
}
// a linear model the scan can follow (sr_ring_tab_build's rule)
inline bool ring_linear_model_ok(int R, float lo, float hi) {
  const float step = (hi - lo) / (float)(R - 1);
  return step >= 0.01f && fabsf(lo) <= 1e4f && fabsf(hi) <= 1e4f;
}

// The table of a built-in model: bound[i] is the first float at which the new value holds (the
// lower bound is inclusive), so the table reproduces ring_id_model on every float in
// [bound[0], bound[n]).  A value outside 0 .. R - 1 becomes -1.  bound [LOAM_RING_TABLE_MAX + 1],
// ring [LOAM_RING_TABLE_MAX]; kRingTableOk, or why not (nothing is written then): the model's own
// fault, or the check's refusal of the table it would give.
inline int ring_table_of_model_why(int model, int R, float lo, float hi, uint32_t* n, float* bound, int32_t* ring) {
  if (!n || !bound || !ring) return kRingTableNull;
  if (R < 2 || R > 64) return kRingTableRings;
  if (model != LOAM_RING_VLP16 && model != LOAM_RING_LINEAR) return kRingTableModel;
  if (model == LOAM_RING_LINEAR && !ring_linear_model_ok(R, lo, hi)) return kRingTableModel;
  RingSteps s;
  if (!ring_steps_scan([&](float a) { return ring_id_model(model, R, lo, hi, a); }, s)) return kRingTableNarrow;
  int i0, i1;
  if (!ring_steps_valid_span(s, R, i0, i1)) return kRingTableEmpty;
  const int m = i1 - i0 + 1;
  if (m > kRingTableMax) return kRingTableN;
  float b[kRingTableMax + 1];
  int32_t r[kRingTableMax];
  for (int k = 0; k <= m; ++k) b[k] = s.first_new[i0 - 1 + k];
  for (int k = 0; k < m; ++k) r[k] = s.val[i0 + k] >= 0 && s.val[i0 + k] <= R - 1 ? s.val[i0 + k] : -1;
  const int why = ring_table_check_why((uint32_t)R, (uint32_t)m, b, r);
  if (why != kRingTableOk) return why;
  *n = (uint32_t)m;
  for (int k = 0; k <= m; ++k) bound[k] = b[k];
  for (int k = 0; k < m; ++k) ring[k] = r[k];
  return kRingTableOk;
}

}  // namespace loam

#endif
