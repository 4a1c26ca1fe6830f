// What more than one of the mapping files (mp.hip, mp_map.hip, mp_loc.hip, mp_commit.hip) needs:
// the device helpers they share and the core's host stages that the others call.  Private to them.
#ifndef LOAM_MP_DEV_HPP
#define LOAM_MP_DEV_HPP

#include "dev_common.hpp"
#include "mp.hpp"
#include "pose_math.hpp"

#pragma GCC visibility push(hidden)
namespace loam {
using namespace loamdev;

constexpr int kMpThreads = 256;

LOAM_D int cube_of(float v, int cen) {  // :446-452, :983-989
  int c = (int)((D(v) + 25.0) / 50.0) + cen;
  if (D(v) + 25.0 < 0) c--;
  return c;
}
LOAM_D int cube_index(int i, int j, int k) { return i + kCubeW * j + kCubeW * kCubeH * k; }

LOAM_D int* slot_table(const MpBuffers& b, int pool, int p) {
  return b.slots + ((size_t)pool * b.P + p) * kCubeNum * 4;
}

// sin / cos of the TobeMapped rotation in double (pointAssociateToMap, :240-257), kept per instance
// in b.rot beside the state: written wherever transformTobeMapped changes (prepare, each L-M
// step, the IMU blend), read by every kernel that maps points.  Per thread they were six double
// sin / cos calls, the larger part of the 5-NN kernel's instructions.
LOAM_D void rot_store(const MpBuffers& b, int p, const float* T) {
  const loampose::MapRot r = loampose::map_rot(T);
  double* d = b.rot + (size_t)p * 6;
  d[0] = r.c0; d[1] = r.s0; d[2] = r.c1; d[3] = r.s1; d[4] = r.c2; d[5] = r.s2;
}
LOAM_D loampose::MapRot rot_load(const MpBuffers& b, int p) {
  const double* d = b.rot + (size_t)p * 6;
  const float* T = b.state + (size_t)p * kMpStateFloats + kMpTobe;
  loampose::MapRot r;
  r.c0 = d[0]; r.s0 = d[1]; r.c1 = d[2]; r.s1 = d[3]; r.c2 = d[4]; r.s2 = d[5];
  r.t3 = T[3]; r.t4 = T[4]; r.t5 = T[5];
  return r;
}

// one thread: the frame's pose prediction for instance p (the odometry pose through the message
// round trip, transformAssociateToMap with the instance's Bef / Aft, :110-197), its rotation and
// the point on the Y axis of the FOV test (:616-622)
LOAM_D void prepare_pose(const MpBuffers& b, const MpInput& in, int p) {
  float* st = b.state + (size_t)p * kMpStateFloats;
  float pose[6] = {0, 0, 0, 0, 0, 0};
  if (in.pose)
    for (int k = 0; k < 6; ++k) pose[k] = in.pose[(size_t)p * in.pose_stride + k];
  loampose::pose_through_msg(pose, st + kMpSum);
  loampose::associate_to_map(st + kMpSum, st + kMpBef, st + kMpAft, st + kMpIncre, st + kMpTobe);
  const float* T = st + kMpTobe;
  const loampose::MapRot r = loampose::map_rot(T);
  rot_store(b, p, T);
  const float4 onY = loampose::point_to_map(r, make_float4(0.0f, 10.0f, 0.0f, 0.0f));
  st[kMpOnY] = onY.x; st[kMpOnY + 1] = onY.y; st[kMpOnY + 2] = onY.z;
}

// thread tid < 125: cube tid of the 5x5x5 neighbourhood of the centre cube (cI, cJ, cK) in the
// reference's i, j, k loop order: inside the grid and in the field of view (:624-672)?  ind: its index
LOAM_D bool fov_cube(const float* st, int tid, int cI, int cJ, int cK, int cW, int cH, int cD, int& ind) {
  const float* T = st + kMpTobe;
  bool inFOV = false;
  ind = 0;
  if (tid < 125) {
    const int i = cI - 2 + tid / 25, j = cJ - 2 + (tid / 5) % 5, k = cK - 2 + tid % 5;
    if (i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD) {
      const float ox = st[kMpOnY], oy = st[kMpOnY + 1], oz = st[kMpOnY + 2];
      const float centerX = (float)(50.0 * (i - cW));
      const float centerY = (float)(50.0 * (j - cH));
      const float centerZ = (float)(50.0 * (k - cD));
      for (int ii = -1; ii <= 1; ii += 2)
        for (int jj = -1; jj <= 1; jj += 2)
          for (int kk = -1; kk <= 1; kk += 2) {
            const float cornerX = (float)(D(centerX) + 25.0 * ii);
            const float cornerY = (float)(D(centerY) + 25.0 * jj);
            const float cornerZ = (float)(D(centerZ) + 25.0 * kk);
            const float sq1 = (T[3] - cornerX) * (T[3] - cornerX) + (T[4] - cornerY) * (T[4] - cornerY) +
                              (T[5] - cornerZ) * (T[5] - cornerZ);
            const float sq2 = (ox - cornerX) * (ox - cornerX) + (oy - cornerY) * (oy - cornerY) +
                              (oz - cornerZ) * (oz - cornerZ);
            const float check1 = (float)(100.0 + D(sq1) - D(sq2) - 10.0 * sqrt(3.0) * sqrt(D(sq1)));
            const float check2 = (float)(100.0 + D(sq1) - D(sq2) + 10.0 * sqrt(3.0) * sqrt(D(sq1)));
            if (check1 < 0 && check2 > 0) inFOV = true;
          }
      ind = cube_index(i, j, k);
    }
  }
  return inFOV;
}

// what the localization kernels read of the streaming store (instance 0's current pool)
struct LocStore {
  const int* slots;     // [kCubeNum][4] (offC, cntC, offS, cntS)
  const float4* pool;
  const int* istate;    // the store's instance state (grid centre, error word)
  int map_cap;
};
inline LocStore loc_store(const MpBuffers& s) {
  LocStore v;
  v.slots = s.slots + (size_t)s.pool_cur * s.P * kCubeNum * 4;
  v.pool = s.pool + (size_t)s.pool_cur * s.P * s.map_cap;
  v.istate = s.istate;
  v.map_cap = s.map_cap;
  return v;
}

// instance p's stacks from its two clouds (nc / ns points, clamped to capC / capS by the caller):
// every point to the map frame and back (:424-434, :683-691), corner at 0, surf at capC of the
// instance's cap_stack segment; then the segment words of the stacks' VoxelGrid.  over(): a count as
// given exceeds its capacity (ERR_CAP_STACK; asked by the one thread that writes the words)
template <class Over>
LOAM_D void stack_body(const MpBuffers& b, int p, const float4* corner, const float4* surf, int nc, int ns, Over over) {
  const loampose::MapRot r = rot_load(b, p);
  float4* out = b.stack2 + (size_t)p * b.cap_stack;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nc + ns; i += gridDim.x * 256) {
    const float4 a = i < nc ? corner[i] : surf[i - nc];
    const float4 m = loampose::point_to_map(r, a);
    out[i < nc ? i : b.capC + (i - nc)] = loampose::point_to_tobe_mapped(r, m);
  }
  if (p == 0 && blockIdx.x == 0 && threadIdx.x == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; }  // (vg_stack's lists)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const size_t base = (size_t)p * b.cap_stack;
    b.sseg_b[p * 2 + 0] = (int)base;
    b.sseg_e[p * 2 + 0] = (int)base + nc;
    b.sseg_b[p * 2 + 1] = (int)(base + b.capC);
    b.sseg_e[p * 2 + 1] = (int)(base + b.capC) + ns;
    b.sseg_leaf[p * 2 + 0] = 0.2f;
    b.sseg_leaf[p * 2 + 1] = 0.4f;
    if (over()) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_STACK;
  }
}

// ---------------------------------------------------------------- the core's host stages (mp.hip)
// k_mp_stack / k_mp_register for the b.P instances of b
void mp_launch_stack(MpBuffers& b, const MpInput& in, hipStream_t st);
void mp_launch_register(MpBuffers& b, const MpInput& in, hipStream_t st);
// the stacks' VoxelGrid (:693-701) on vs (k_mp_stack zeroed the cascade's list counters)
void mp_stack_vg(MpBuffers& b, int P, hipStream_t vs, int stack_max);
// the 1 m voxel hashes of FromMap's corner and surf parts; spread: the grid-per-cloud build
void mp_hash_from(MpBuffers& b, int P, hipStream_t st, bool spread = false);
// k_mp_lm_begin, the iterations, k_mp_lm_end; persist: one instance may take the persistent launch
void mp_lm_loop(MpBuffers& b, int P, hipStream_t st, Prof* prof, bool map_empty, bool persist);
// A working set's two allocation groups, each spelt once (errors collect in A; the caller frees):
// the solve part of P instances (b.capC / b.capS / b.cap_stack set; the VoxelGrid scratch sorts
// vg_pts points and lists vg_segs segments), its state, istate, done and ls_epoch zeroed ...
void mp_alloc_solve(DevAlloc& A, MpBuffers& b, int P, size_t vg_pts, size_t vg_segs);
// ... and the FromMap part of P instances of cap points (sets b.map_cap and b.tmax)
void mp_alloc_from(DevAlloc& A, MpBuffers& b, int P, int cap);

}  // namespace loam
#pragma GCC visibility pop
#endif
