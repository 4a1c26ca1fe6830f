// Host check (tests/test_ring_table.py): csrc/ring_table.hpp in a stand-alone program under
// AddressSanitizer / UBSan, compiled as plain C++ (the header makes no HIP call).
//  - ring_table_check_why: every refusal, and the acceptances at the limits (n = 1 and 64, a width
//    just under and just at 1/32 degree, ring = -1 and ring = n_rings - 1);
//  - ring_table_of_model_why for VLP-16 (R = 16) and the linear model (R = 64, -24.8 / 2.0): the
//    table equals ring_id_model on every neighbouring float within 8 ulp of each bound and on a
//    1e-3 degree sweep between the ends; VLP-16's bounds are the half-integers (inclusive below for
//    positive angles, the next float above for negative ones);
//  - a model of more than 64 intervals and a linear model with a step under 1/32 degree are refused
//    and write nothing.
// Prints "<cases> <wrong>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/ring_table.hpp"

using namespace loam;

static long cases = 0, wrong = 0;
static void expect(bool ok, const char* what) {
  ++cases;
  if (!ok) {
    ++wrong;
    fprintf(stderr, "wrong: %s\n", what);
  }
}

// exactly n + 1 bounds and n rings on the heap, so that a read past either is the sanitizer's
struct Table {
  std::vector<float> b;
  std::vector<int32_t> r;
  Table(int n, float first, float width) : b(n + 1), r(n) {
    for (int i = 0; i <= n; ++i) b[i] = first + width * (float)i;
    for (int i = 0; i < n; ++i) r[i] = i % 16;
  }
  int why(uint32_t n_rings = 16) const { return ring_table_check_why(n_rings, (uint32_t)r.size(), b.data(), r.data()); }
};

static void check_the_check() {
  expect(Table(1, -1.0f, 2.0f).why() == kRingTableOk, "n = 1");
  expect(Table(64, -32.0f, 1.0f).why() == kRingTableOk, "n = 64");
  {
    Table t(65, -32.0f, 0.5f);  // (n beyond the limit is refused before anything is read)
    expect(t.why() == kRingTableN, "n = 65");
    expect(ring_table_check_why(16, 0, t.b.data(), t.r.data()) == kRingTableN, "n = 0");
  }
  {
    Table t(4, 0.0f, 1.0f);
    expect(ring_table_check_why(16, 4, nullptr, t.r.data()) == kRingTableNull, "null bounds");
    expect(ring_table_check_why(16, 4, t.b.data(), nullptr) == kRingTableNull, "null rings");
    expect(t.why(1) == kRingTableRings && t.why(65) == kRingTableRings, "n_rings out of range");
    expect(t.why(2) == kRingTableRing, "ring = n_rings");
    expect(t.why(4) == kRingTableOk, "ring = n_rings - 1");
  }
  for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 89.0f, 120.0f}) {
    Table t(4, 0.0f, 1.0f);
    t.b[4] = bad;
    expect(t.why() == kRingTableBound, "a bound not finite or not below 89");
    Table u(4, 0.0f, 1.0f);
    u.b[0] = -bad;
    expect(u.why() == kRingTableBound, "a bound not finite or not above -89");
  }
  {
    Table t(2, 0.0f, 1.0f);
    t.b[0] = std::nextafterf(-89.0f, 0.0f);
    t.b[2] = std::nextafterf(89.0f, 0.0f);
    expect(t.why() == kRingTableOk, "bounds just inside (-89, 89)");
  }
  {
    Table t(4, 0.0f, 1.0f);
    t.b[2] = t.b[1];
    expect(t.why() == kRingTableOrder, "equal bounds");
    t.b[2] = 0.5f;
    expect(t.why() == kRingTableOrder, "descending bounds");
  }
  {
    Table t(4, 0.0f, 1.0f);
    t.b[2] = 1.0f + 0.03125f;  // exactly 1/32 above b[1]
    expect(t.why() == kRingTableOk, "a width of exactly 1/32 degree");
    t.b[2] = std::nextafterf(1.0f + 0.03125f, 0.0f);
    expect(t.why() == kRingTableNarrow, "a width just under 1/32 degree");
  }
  {
    Table t(4, 0.0f, 1.0f);
    t.r[1] = -1;
    expect(t.why() == kRingTableOk, "ring = -1");
    t.r[1] = -2;
    expect(t.why() == kRingTableRing, "ring = -2");
    for (auto& v : t.r) v = -1;
    expect(t.why() == kRingTableEmpty, "every ring -1");
  }
  {  // the lookup's rule on a table with a dropped interval
    Table t(3, -1.0f, 1.0f);  // bounds -1, 0, 1, 2
    t.r = {5, -1, 7};
    auto L = [&](float a) { return ring_table_lookup(t.b.data(), t.r.data(), 3, a); };
    expect(L(-1.0f) == 5 && L(std::nextafterf(0.0f, -1.0f)) == 5 && L(0.0f) == -1 && L(0.5f) == -1 && L(1.0f) == 7,
           "inclusive lower bounds");
    expect(L(std::nextafterf(-1.0f, -2.0f)) == -1 && L(2.0f) == -1 && L(std::nextafterf(2.0f, 0.0f)) == 7 &&
               L(std::numeric_limits<float>::quiet_NaN()) == -1 && L(-std::numeric_limits<float>::infinity()) == -1,
           "outside and NaN are dropped");
  }
  for (int n = 1; n <= 64; ++n) {  // every n: each interval's two end floats and its middle
    Table t(n, -30.0f, 0.9f);
    for (int i = 0; i < n; ++i) t.r[i] = i;
    bool ok = true;
    for (int i = 0; i < n; ++i)
      for (float a : {t.b[i], 0.5f * (t.b[i] + t.b[i + 1]), std::nextafterf(t.b[i + 1], -90.0f)})
        ok = ok && ring_table_lookup(t.b.data(), t.r.data(), n, a) == i;
    expect(ok, "the lookup finds every interval of every table size");
  }
}

static float step_ulps(float a, int k) {
  for (; k > 0; --k) a = std::nextafterf(a, 90.0f);
  for (; k < 0; ++k) a = std::nextafterf(a, -90.0f);
  return a;
}

static void check_model(int model, int R, float lo, float hi, uint32_t want_n) {
  std::vector<float> b(LOAM_RING_TABLE_MAX + 1);
  std::vector<int32_t> r(LOAM_RING_TABLE_MAX);
  uint32_t n = 0;
  const int why = ring_table_of_model_why(model, R, lo, hi, &n, b.data(), r.data());
  expect(why == kRingTableOk && n == want_n, "the model's table is built");
  if (why != kRingTableOk) return;
  expect(ring_table_check_why((uint32_t)R, n, b.data(), r.data()) == kRingTableOk, "and passes the check");
  auto model_ring = [&](float a) {
    const int v = ring_id_model(model, R, lo, hi, a);
    return v >= 0 && v <= R - 1 ? v : -1;
  };
  long bad = 0;
  for (uint32_t i = 0; i <= n; ++i)
    for (int k = -8; k <= 8; ++k) {
      const float a = step_ulps(b[i], k);
      if (a < b[0] || a >= b[n]) {  // beyond the ends the table drops; the model has no valid ring there either
        bad += ring_table_lookup(b.data(), r.data(), (int)n, a) != -1 || model_ring(a) != -1;
        continue;
      }
      bad += ring_table_lookup(b.data(), r.data(), (int)n, a) != model_ring(a);
    }
  expect(bad == 0, "table == ring_id within 8 ulp of every bound");
  bad = 0;
  long swept = 0;
  for (double a = (double)b[0]; a < (double)b[n]; a += 1e-3, ++swept)
    bad += ring_table_lookup(b.data(), r.data(), (int)n, (float)a) != model_ring((float)a);
  expect(bad == 0 && swept > 26000, "table == ring_id on a 1e-3 degree sweep");
  if (model == LOAM_RING_VLP16) {
    bool ok = n == 31;
    for (uint32_t i = 0; i <= n && ok; ++i) {
      const float h = -15.5f + (float)i;
      ok = b[i] == (h > 0.0f ? h : std::nextafterf(h, 90.0f));
    }
    expect(ok, "VLP-16 bounds are the half-integers");
    expect(r[0] == 0 && r[14] == 14 && r[15] == 15 && r[16] == 1 && r[30] == 15, "VLP-16 rings");
  }
}

static void check_refused_models() {
  std::vector<float> b(LOAM_RING_TABLE_MAX + 1, 777.0f);
  std::vector<int32_t> r(LOAM_RING_TABLE_MAX, 777);
  uint32_t n = 777;
  auto untouched = [&] {
    bool ok = n == 777;
    for (float v : b) ok = ok && v == 777.0f;
    for (int32_t v : r) ok = ok && v == 777;
    return ok;
  };
  // VLP-16's rule with 64 rings: 127 intervals between -63.5 and 63.5
  expect(ring_table_of_model_why(LOAM_RING_VLP16, 64, 0, 0, &n, b.data(), r.data()) == kRingTableN && untouched(),
         "more than 64 intervals");
  // linear, R = 64, step (0.5 + 1.0) / 63 = 0.0238 < 1/32 degree
  expect(ring_table_of_model_why(LOAM_RING_LINEAR, 64, -1.0f, 0.5f, &n, b.data(), r.data()) == kRingTableNarrow && untouched(),
         "a linear step under 1/32 degree");
  expect(ring_table_of_model_why(LOAM_RING_LINEAR, 64, 2.0f, 2.0f, &n, b.data(), r.data()) == kRingTableModel && untouched(),
         "a degenerate linear model");
  expect(ring_table_of_model_why(LOAM_RING_TABLE, 16, 0, 0, &n, b.data(), r.data()) == kRingTableModel && untouched(),
         "not a built-in model");
  expect(ring_table_of_model_why(LOAM_RING_VLP16, 16, 0, 0, nullptr, b.data(), r.data()) == kRingTableNull, "null n");
}

int main() {
  check_the_check();
  check_model(LOAM_RING_VLP16, 16, -24.8f, 2.0f, 31);
  check_model(LOAM_RING_LINEAR, 64, -24.8f, 2.0f, 64);
  check_refused_models();
  printf("%ld %ld\n", cases, wrong);
  return wrong ? 1 : 0;
}
