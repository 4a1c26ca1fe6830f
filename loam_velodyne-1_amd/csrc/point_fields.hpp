// Ring and time from a sweep's own fields (loam_set_point_fields): the rules of the
// check, the extraction of a field from a record, the conversion of a time value and the word a
// point carries in the fourth component of a raw float4.  No HIP call, so the header compiles into
// a stand-alone program (tests/point_fields_check.cpp); the extraction, the conversion and the word
// are shared with the device push's gather (lanes.hip), which makes the host and the device forms
// one statement of the arithmetic.
#ifndef LOAM_POINT_FIELDS_HPP
#define LOAM_POINT_FIELDS_HPP

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/loam/loam.h"

#ifdef __HIPCC__
#define LOAM_PF_HD __host__ __device__ __forceinline__
#else
#define LOAM_PF_HD inline
#endif

namespace loam {

// the word of a dropped point: any negative value drops, this is the one written
constexpr float kPointDropped = -1.0f;
constexpr uint32_t kFieldEndMax = 65536;  // a field ends at or below this byte of a record

// A context's fields as the packing code reads them: loam_point_fields with the map copied in
// (map_n = 0: identity) and n_rings beside it.  on = 0: the ring model or table rules.
struct PointFields {
  uint32_t on = 0;
  uint32_t ring_type = 0, ring_offset = 0, time_type = 0, time_offset = 0;
  uint32_t map_n = 0, n_rings = 0;
  uint32_t end = 0;  // the larger end of the two fields: the least stride_bytes of a cloud
  double time_scale = 1.0, time_bias = 0.0;
  int16_t map[LOAM_RING_MAP_MAX];
};

LOAM_PF_HD uint32_t field_size(uint32_t type) {
  return type == LOAM_FIELD_U8 ? 1u
         : type == LOAM_FIELD_U16 ? 2u
         : (type == LOAM_FIELD_U32 || type == LOAM_FIELD_F32) ? 4u
         : type == LOAM_FIELD_F64 ? 8u
                                  : 0u;
}

// ---------------------------------------------------------------- the check
enum {
  kFieldsOk = 0,
  kFieldsNull,       // f is null
  kFieldsRingType,   // ring_type not U8 | U16 | U32
  kFieldsTimeType,   // time_type not NONE | F32 | U32 | F64
  kFieldsOffset,     // an offset below 12 or not a multiple of the field's size
  kFieldsEnd,        // a field ends beyond byte 65536 of a record
  kFieldsOverlap,    // the two fields overlap
  kFieldsScale,      // time_scale / time_bias not finite, or time_scale == 0
  kFieldsMapNull,    // ring_map == NULL with ring_map_n != 0
  kFieldsMapN,       // a map of 0 or more than LOAM_RING_MAP_MAX entries
  kFieldsMapRing,    // a map entry outside [-1, n_rings)
  kFieldsMapEmpty,   // every map entry is -1
  kFieldsRings       // n_rings outside [2, 64]
};

inline int point_fields_check_why(uint32_t n_rings, const loam_point_fields* f) {
  if (!f) return kFieldsNull;
  if (n_rings < 2 || n_rings > 64) return kFieldsRings;
  if (f->ring_type != LOAM_FIELD_U8 && f->ring_type != LOAM_FIELD_U16 && f->ring_type != LOAM_FIELD_U32)
    return kFieldsRingType;
  if (f->time_type != LOAM_FIELD_NONE && f->time_type != LOAM_FIELD_F32 && f->time_type != LOAM_FIELD_U32 &&
      f->time_type != LOAM_FIELD_F64)
    return kFieldsTimeType;
  const bool timed = f->time_type != LOAM_FIELD_NONE;
  const uint32_t rs = field_size(f->ring_type), ts = field_size(f->time_type);
  if (f->ring_offset < 12 || f->ring_offset % rs != 0) return kFieldsOffset;
  if (timed && (f->time_offset < 12 || f->time_offset % ts != 0)) return kFieldsOffset;
  if ((uint64_t)f->ring_offset + rs > kFieldEndMax) return kFieldsEnd;
  if (timed && (uint64_t)f->time_offset + ts > kFieldEndMax) return kFieldsEnd;
  if (timed && f->ring_offset < f->time_offset + ts && f->time_offset < f->ring_offset + rs) return kFieldsOverlap;
  if (timed && (!std::isfinite(f->time_scale) || !std::isfinite(f->time_bias) || f->time_scale == 0.0)) return kFieldsScale;
  if (!f->ring_map) return f->ring_map_n == 0 ? kFieldsOk : kFieldsMapNull;
  if (f->ring_map_n < 1 || f->ring_map_n > LOAM_RING_MAP_MAX) return kFieldsMapN;
  bool any = false;
  for (uint32_t i = 0; i < f->ring_map_n; ++i) {
    if (f->ring_map[i] < -1 || f->ring_map[i] >= (int32_t)n_rings) return kFieldsMapRing;
    any = any || f->ring_map[i] >= 0;
  }
  return any ? kFieldsOk : kFieldsMapEmpty;
}

inline const char* point_fields_why_text(int why) {
  switch (why) {
    case kFieldsOk: return "ok";
    case kFieldsNull: return "null argument";
    case kFieldsRingType: return "ring_type must be LOAM_FIELD_U8, U16 or U32";
    case kFieldsTimeType: return "time_type must be LOAM_FIELD_NONE, F32, U32 or F64";
    case kFieldsOffset: return "every offset must be at least 12 and a multiple of its field's size";
    case kFieldsEnd: return "every field must end at or below byte 65536";
    case kFieldsOverlap: return "the ring and time fields must not overlap";
    case kFieldsScale: return "time_scale and time_bias must be finite and time_scale not 0";
    case kFieldsMapNull: return "ring_map is null but ring_map_n is not 0";
    case kFieldsMapN: return "ring_map_n must be in [1, LOAM_RING_MAP_MAX]";
    case kFieldsMapRing: return "every ring_map entry must be in [-1, n_rings)";
    case kFieldsMapEmpty: return "at least one ring_map entry must not be -1";
    default: return "n_rings must be in [2, 64]";
  }
}

// f (which the check has passed) as the packing code reads it
inline PointFields point_fields_of(uint32_t n_rings, const loam_point_fields& f) {
  PointFields p;
  p.on = 1;
  p.ring_type = f.ring_type;
  p.ring_offset = f.ring_offset;
  p.time_type = f.time_type;
  p.time_offset = f.time_type != LOAM_FIELD_NONE ? f.time_offset : 0;
  p.time_scale = f.time_scale;
  p.time_bias = f.time_bias;
  p.n_rings = n_rings;
  p.map_n = f.ring_map ? f.ring_map_n : 0;
  for (uint32_t i = 0; i < (uint32_t)LOAM_RING_MAP_MAX; ++i) p.map[i] = i < p.map_n ? (int16_t)f.ring_map[i] : (int16_t)-1;
  p.end = f.ring_offset + field_size(f.ring_type);
  if (f.time_type != LOAM_FIELD_NONE && f.time_offset + field_size(f.time_type) > p.end)
    p.end = f.time_offset + field_size(f.time_type);
  return p;
}

// ---------------------------------------------------------------- a point's word
// the ring of field value v: -1 for a value beyond the map (or beyond n_rings without one) and
// where the map says -1
LOAM_PF_HD int field_ring(uint32_t v, uint32_t map_n, const int16_t* map, uint32_t n_rings) {
  if (map_n == 0) return v < n_rings ? (int)v : -1;
  return v < map_n ? (int)map[v] : -1;
}

// tau of a time value already widened to double: the product rounded to double, the sum rounded
// to double, the result rounded to float (the build has -ffp-contract=off: no fused multiply-add)
LOAM_PF_HD float field_tau(double t, double scale, double bias) {
  const double prod = t * scale;
  const double sum = prod + bias;
  return (float)sum;
}

// whether a point with this tau is kept: finite and 0 <= tau <= 0.5 (-0.0 is kept, a NaN is not)
LOAM_PF_HD bool field_tau_kept(float tau) { return tau >= 0.0f && tau <= 0.5f; }

// The word of a point whose coordinates are finite: (float)r in ring-only mode (timed = false),
// (float)r + tau in ring-and-time mode, kPointDropped for a dropped point.  tau <= 0.5 keeps
// (int)word == r, and word - (float)r gives tau back exactly.
LOAM_PF_HD float field_word(int r, bool timed, float tau) {
  if (r < 0) return kPointDropped;
  if (!timed) return (float)r;
  if (!field_tau_kept(tau)) return kPointDropped;
  return (float)r + tau;
}

// ---------------------------------------------------------------- extraction (host: any alignment)
inline uint32_t field_load_uint(const unsigned char* rec, uint32_t type, uint32_t off) {
  if (type == LOAM_FIELD_U8) return rec[off];
  if (type == LOAM_FIELD_U16) {
    uint16_t v;
    std::memcpy(&v, rec + off, 2);
    return v;
  }
  uint32_t v;
  std::memcpy(&v, rec + off, 4);
  return v;
}
inline double field_load_time(const unsigned char* rec, uint32_t type, uint32_t off) {
  if (type == LOAM_FIELD_F32) {
    float v;
    std::memcpy(&v, rec + off, 4);
    return (double)v;
  }
  if (type == LOAM_FIELD_F64) {
    double v;
    std::memcpy(&v, rec + off, 8);
    return v;
  }
  return (double)field_load_uint(rec, LOAM_FIELD_U32, off);
}
// the word of the record at rec (the coordinates are the caller's business)
inline float field_word_of_record(const PointFields& p, const unsigned char* rec) {
  const int r = field_ring(field_load_uint(rec, p.ring_type, p.ring_offset), p.map_n, p.map, p.n_rings);
  const bool timed = p.time_type != LOAM_FIELD_NONE;
  const float tau = timed ? field_tau(field_load_time(rec, p.time_type, p.time_offset), p.time_scale, p.time_bias) : 0.0f;
  return field_word(r, timed, tau);
}

// ---------------------------------------------------------------- extraction from aligned dwords
// (the device push: records at a 4-byte aligned address with a 4-byte multiple stride)
// a sub-dword field from the dword that holds it (offsets are multiples of the field's size, so a
// field never straddles two dwords)
LOAM_PF_HD uint32_t field_uint_of_dword(uint32_t dword, uint32_t type, uint32_t off) {
  if (type == LOAM_FIELD_U8) return (dword >> (8 * (off & 3))) & 0xffu;
  if (type == LOAM_FIELD_U16) return (dword >> (8 * (off & 2))) & 0xffffu;
  return dword;
}
// a time value from its dword(s): lo at the field's offset, hi the next one (F64 only; its address
// may be 4 mod 8)
LOAM_PF_HD double field_time_of_dwords(uint32_t lo, uint32_t hi, uint32_t type) {
  if (type == LOAM_FIELD_F32) return (double)__builtin_bit_cast(float, lo);
  if (type == LOAM_FIELD_F64) return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
  return (double)lo;
}

}  // namespace loam
#endif
