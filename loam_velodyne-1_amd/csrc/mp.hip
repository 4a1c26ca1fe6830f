// Laser mapping on gfx950: the laserMapping loop body (/root/reference/src/laserMapping.cpp:411-1097)
// for P independent map instances (the streaming map, or one per config-4 problem).
//
//  k_mp_prepare    pose prediction (transformAssociateToMap :110-197, fed through the nav_msgs
//                  quaternion round trip :304-321), cube-grid recentring (:440-614) as slot-table
//                  shifts, FOV cube selection (:616-672), FromMap prefix.
//  k_mp_stack      stack to map frame and back (:424-434, :683-691, Q24)
//  vg_run          segmented PCL VoxelGrid for the stacks (:693-701) and the valid cubes (:1018-1036): vg.hip
//  k_mp_gather     FromMap = valid cubes concatenated (:674-681), then voxel-hashed (k_hash_build)
//  k_mp_nnfit      one L-M iteration for every instance at once, lane per stack point: the exact
//                  5-NN (:714-719, :821-826) through the 1 m hash (any point within the 1 m acceptance
//                  radius lies in the 27 cells; cells pruned by box distance), the corner PCA with the
//                  3x3 Jacobi / surface 5x3 QR plane (reused while the ordered 5-NN is unchanged),
//                  weight -> accepted row (:721-877), and (fused) the fp64 JᵀJ / Jᵀb partials with
//                  the 6x6 step in the instance's last workgroup (:879-974)
//  k_mp_iter       the step as its own launch (tuning mp_fused_max)
//  k_mp_lm_small / k_mp_lm_stream   the same for a few instances / one (streaming)
//  k_mp_lm_end     transformUpdate (:199-232)
//  k_mp_insert     stack -> cubes in stack order (:980-1016)
//  k_mp_vcopy      per valid cube: old content ++ appended points -> DS input
//  k_mp_compact    new cube store (valid cubes downsampled, others appended) into the other pool
//  k_mp_register   full cloud to the map frame (:1060-1063)
// The other mapping services are files of their own: mp_map.hip (export / import,
// k_mp_map_*), mp_loc.hip (localization and the shared lanes' frame, k_mp_loc_*), mp_commit.hip (the
// shared lanes' commit, k_cm_*), mp_nn5_hook.hip (the 5-NN hook, k_dev_nn5_*); mp_dev.hpp holds what
// they share with this file, mp_nn.hpp the 5-NN search.

#include <algorithm>
#include <functional>
#include <cstring>
#include <vector>

#include "mp_nn.hpp"

using namespace loamdev;

namespace loam {
#ifdef LOAM_PHASES
__device__ PhaseAcc g_ph_mp = {~0ull, 0ull, 0ull, {{0}}};
#endif

namespace {
__global__ __launch_bounds__(kMpThreads) void k_mp_prepare(MpBuffers b, MpInput in) {
  const int p = blockIdx.x, tid = threadIdx.x;
  float* st = b.state + (size_t)p * kMpStateFloats;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  int* slots = slot_table(b, b.pool_cur, p);
  __shared__ int sh_shift[3], sh_count[3];
  __shared__ int sh_nshift, sh_c[3], sh_cen[3], sh_scan[16];
  if (tid == 0) {
    prepare_pose(b, in, p);
    const float* T = st + kMpTobe;
    int cW = ist[kMiCenW], cH = ist[kMiCenH], cD = ist[kMiCenD];
    int cI = cube_of(T[3], cW), cJ = cube_of(T[4], cH), cK = cube_of(T[5], cD);
    // :454-614: each `while` moves the grid one slab per pass until the centre cube is >= 3 from
    // the edge.  The pass counts are closed-form; a line of cubes shifted by its full length (or
    // more) is entirely cleared, so at most that many slot-table shifts are replayed per axis
    // while the centre indices take every pass (ist[kMiShifts] counts the reference's passes).
    const int dim[3] = {kCubeW, kCubeH, kCubeD};
    int* c[3] = {&cI, &cJ, &cK};
    int* cen[3] = {&cW, &cH, &cD};
    int n = 0;
    long long passes = 0;
    for (int axis = 0; axis < 3; ++axis) {
      long long up = 0, down = 0;
      if (*c[axis] < 3) up = 3 - (long long)*c[axis];
      else if (*c[axis] >= dim[axis] - 3) down = (long long)*c[axis] - (dim[axis] - 4);
      const long long moves = up ? up : down;
      if (moves) {
        *c[axis] += (int)(up - down);
        *cen[axis] += (int)(up - down);
        sh_shift[n] = axis * 2 + (up ? 1 : 0);
        sh_count[n] = (int)(moves < dim[axis] ? moves : dim[axis]);
        ++n;
        passes += moves;
      }
    }
    ist[kMiShifts] = (int)(passes < 0x7fffffff ? passes : 0x7fffffff);
    sh_nshift = n;
    sh_c[0] = cI; sh_c[1] = cJ; sh_c[2] = cK;
    ist[kMiCubeI] = cI; ist[kMiCubeJ] = cJ; ist[kMiCubeK] = cK;
    ist[kMiCenW] = cW; ist[kMiCenH] = cH; ist[kMiCenD] = cD;
    sh_cen[0] = cW; sh_cen[1] = cH; sh_cen[2] = cD;
  }
  __syncthreads();
  for (int s = 0; s < sh_nshift; ++s)
  for (int rep = 0; rep < sh_count[s]; ++rep) {  // slot-table shifts: the cleared cube wraps around
    const int axis = sh_shift[s] >> 1, up = sh_shift[s] & 1;
    const int nAx = axis == 0 ? kCubeW : (axis == 1 ? kCubeH : kCubeD);
    const int na = axis == 0 ? kCubeH : kCubeW, nb = axis == 2 ? kCubeH : kCubeD;
    for (int line = tid; line < na * nb; line += kMpThreads) {
      const int a = line % na, bb = line / na;
      auto at = [&](int c) {
        if (axis == 0) return cube_index(c, a, bb);
        if (axis == 1) return cube_index(a, c, bb);
        return cube_index(a, bb, c);
      };
      int4* sl = (int4*)slots;
      if (up) {
        int4 keep = sl[at(nAx - 1)];
        for (int c = nAx - 1; c >= 1; --c) sl[at(c)] = sl[at(c - 1)];
        keep.y = 0; keep.w = 0;
        sl[at(0)] = keep;
      } else {
        int4 keep = sl[at(0)];
        for (int c = 0; c < nAx - 1; ++c) sl[at(c)] = sl[at(c + 1)];
        keep.y = 0; keep.w = 0;
        sl[at(nAx - 1)] = keep;
      }
    }
    __threadfence_block();  // (one workgroup: the next shift's lines are other threads')
    __syncthreads();
  }
  // FOV selection (:616-672) and FromMap prefix: thread c tests cube c of the 5x5x5
  // neighbourhood (the reference's i, j, k loop order), block scans keep that order
  int ind;
  const bool inFOV = fov_cube(st, tid, sh_c[0], sh_c[1], sh_c[2], sh_cen[0], sh_cen[1], sh_cen[2], ind);
  const int nC = inFOV ? slots[ind * 4 + 1] : 0, nS = inFOV ? slots[ind * 4 + 3] : 0;
  int nv, accC, accS;
  const int xv = block_excl_scan<kMpThreads>(inFOV ? 1 : 0, sh_scan, nv);
  const int xc = block_excl_scan<kMpThreads>(nC, sh_scan, accC);
  const int xs = block_excl_scan<kMpThreads>(nS, sh_scan, accS);
  int* vp = b.vpre + (size_t)p * (kMaxValid + 1) * 2;
  if (inFOV) {
    b.valid[(size_t)p * kMaxValid + xv] = ind;
    vp[xv * 2 + 0] = xc;
    vp[xv * 2 + 1] = xs;
  }
  if (tid == 0) {
    vp[nv * 2 + 0] = accC;
    vp[nv * 2 + 1] = accS;
    ist[kMiNValid] = nv;
    if (accC + accS > b.map_cap) {
      ist[kMiErr] |= ERR_CAP_MAP;
      accC = accS = 0;
      ist[kMiNValid] = 0;
    }
    b.nfrom[p * 2 + 0] = accC;
    b.nfrom[p * 2 + 1] = accS;
  }
}

// ---------------------------------------------------------------- stacks
__global__ __launch_bounds__(256) void k_mp_stack(MpBuffers b, MpInput in) {
  const int p = blockIdx.y;
  const int nc = min(in.ncorner[p * in.ncorner_stride], b.capC);
  const int ns = min(in.nsurf[p * in.nsurf_stride], b.capS);
  stack_body(b, p, in.corner + (size_t)p * in.corner_stride, in.surf + (size_t)p * in.surf_stride, nc, ns, [&] {
    return in.ncorner[p * in.ncorner_stride] > b.capC || in.nsurf[p * in.nsurf_stride] > b.capS;
  });
}

// ---------------------------------------------------------------- FromMap gather
__global__ __launch_bounds__(256) void k_mp_gather(MpBuffers b) {
  const int p = blockIdx.y;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* vp = b.vpre + (size_t)p * (kMaxValid + 1) * 2;
  const int* slots = slot_table(b, b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  const int totC = vp[nv * 2 + 0], totS = vp[nv * 2 + 1];
  float4* out = b.from + (size_t)p * b.map_cap;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < totC + totS; i += gridDim.x * 256) {
    const int kind = i < totC ? 0 : 1;
    const int t = kind ? i - totC : i;
    int lo = 0, hi = nv - 1;   // last valid cube with prefix <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (vp[mid * 2 + kind] <= t) lo = mid; else hi = mid - 1;
    }
    const int ind = b.valid[(size_t)p * kMaxValid + lo];
    out[i] = pool[slots[ind * 4 + 2 * kind] + (t - vp[lo * 2 + kind])];
  }
}

}  // namespace

__global__ void k_mp_lm_begin(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b.P) return;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  const int nfc = b.nfrom[p * 2 + 0], nfs = b.nfrom[p * 2 + 1];
  ist[kMiStackC] = b.sseg_cnt[p * 2 + 0];
  ist[kMiStackS] = b.sseg_cnt[p * 2 + 1];
  ist[kMiFromC] = nfc;
  ist[kMiFromS] = nfs;
  ist[kMiLmRan] = (nfc > 10 && nfs > 100) ? 1 : 0;  // :706
  ist[kMiStop] = 0;
  ist[kMiIters] = 0;
  ist[kMiRows] = 0;
  ist[kMiRowsLast] = 0;
  ist[kMiFits] = 0;
  ist[kMiDegSteps] = 0;
  ist[kMiNnCand] = 0;
  ist[kMiNnCells] = 0;
  if (p == 0 && b.P == 1) ++b.ls_epoch[0];  // (k_mp_lm_stream's publication words)
}

// One L-M iteration's correspondences (:714-877), lane per stack point (corner, then surf), in
// per-query pieces shared by the batch kernel (k_mp_nnfit) and the small-batch / streaming kernels
// (k_mp_lm_small, k_mp_lm_stream).
//   mp_nn_query   the point at the current TobeMapped pose and its exact 5-NN (seeded with the
//                 previous iteration's), stored in q_nn
//   mp_fit_query  the line (corner PCA, 3x3 Jacobi) or plane (5x3 QR) through the 5 neighbours and
//                 the weighted residual.  A fit depends on nothing but the ordered 5 neighbours, so
//                 it is kept per query and reused while the ordered 5-NN is unchanged from the
//                 previous iteration (bit-identical to refitting)
//   mp_row_accum  the accepted row's J (:897-921) added in fp64
//   mp_step       the 6x6 step on the summed normal equations (:922-974)
namespace {
// the ordered 5-NN a fit was made for, and the fit: corner (x1, y1, z1, valid), (x2, y2, z2, -);
// surf (pa, pb, pc, pd), (valid, -, -, -)
struct MpFit {
  int4 n0, n1;
  float4 g0, g1;
};

// the line (corner: PCA of the 5 neighbours, 3x3 Jacobi, :721-760) or plane (surf: 5x3 QR, :828-850)
// through the ordered 5-NN points nb; jw: this lane's 27 words of LDS scratch for the Jacobi
LOAM_D void mp_fit_compute(bool corner, const float4 (&nb)[5], float* jw, float4& g0, float4& g1) {
  if (corner) {  // :721-760
    float cx = 0, cy = 0, cz = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { cx += nb[k].x; cy += nb[k].y; cz += nb[k].z; }
    cx /= 5; cy /= 5; cz /= 5;
    float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float ax = nb[k].x - cx, ay = nb[k].y - cy, az = nb[k].z - cz;
      a11 += ax * ax; a12 += ax * ay; a13 += ax * az;
      a22 += ay * ay; a23 += ay * az; a33 += az * az;
    }
    a11 /= 5; a12 /= 5; a13 /= 5; a22 /= 5; a23 /= 5; a33 /= 5;
    (void)jw;
    const float A1[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33};
    float D1[3], V1[9];
    loamla::jacobi3_reg(A1, D1, V1);  // (bit-identical to jacobi<3>: tests/test_jacobi3.py)
    const bool valid = D1[0] > 3 * D1[1];
    g0 = make_float4((float)(D(cx) + 0.1 * D(V1[0])), (float)(D(cy) + 0.1 * D(V1[1])),
                     (float)(D(cz) + 0.1 * D(V1[2])), valid ? 1.0f : 0.0f);
    g1 = make_float4((float)(D(cx) - 0.1 * D(V1[0])), (float)(D(cy) - 0.1 * D(V1[1])),
                     (float)(D(cz) - 0.1 * D(V1[2])), 0.0f);
  } else {  // :828-850
    float A0[15], B0[5] = {-1, -1, -1, -1, -1}, X0[3], ws[14];
#pragma unroll
    for (int k = 0; k < 5; ++k) { A0[k * 3 + 0] = nb[k].x; A0[k * 3 + 1] = nb[k].y; A0[k * 3 + 2] = nb[k].z; }
    loamla::qr_solve(A0, B0, 5, 3, X0, ws);
    float pa = X0[0], pb = X0[1], pc = X0[2], pd = 1;
    const float ps = (float)sqrt(D(pa * pa + pb * pb + pc * pc));
    pa /= ps; pb /= ps; pc /= ps; pd /= ps;
    bool planeValid = true;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (fabs(D(pa * nb[k].x + pb * nb[k].y + pc * nb[k].z + pd)) > 0.2) planeValid = false;
    g0 = make_float4(pa, pb, pc, pd);
    g1 = make_float4(planeValid ? 1.0f : 0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// the weighted residual of the mapped point sel against a fit (:762-816 corner, :852-874 surf)
LOAM_D void mp_fit_residual(bool corner, float4 g0, float4 g1, float4 sel, float4& cf, int& ok) {
  ok = 0;
  cf = make_float4(0, 0, 0, 0);
  if (corner && g0.w != 0.0f) {  // :762-816
    const float x0 = sel.x, y0 = sel.y, z0 = sel.z;
    const float x1 = g0.x, y1 = g0.y, z1 = g0.z, x2 = g1.x, y2 = g1.y, z2 = g1.z;
    const float m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1);
    const float m22 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1);
    const float m33 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1);
    const float a012 = (float)sqrt(D(m11 * m11 + m22 * m22 + m33 * m33));
    const float l12 = (float)sqrt(D((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2)));
    const float la = ((y1 - y2) * m11 + (z1 - z2) * m22) / a012 / l12;
    const float lb = -((x1 - x2) * m11 - (z1 - z2) * m33) / a012 / l12;
    const float lc = -((x1 - x2) * m22 + (y1 - y2) * m33) / a012 / l12;
    const float ld2 = a012 / l12;
    const float sw = (float)(1 - 0.9 * fabs(D(ld2)));
    cf = make_float4(sw * la, sw * lb, sw * lc, sw * ld2);
    ok = D(sw) > 0.1 ? 1 : 0;
  } else if (!corner && g1.x != 0.0f) {  // :852-874
    const float pa = g0.x, pb = g0.y, pc = g0.z, pd = g0.w;
    const float pd2 = pa * sel.x + pb * sel.y + pc * sel.z + pd;
    const float sw = (float)(1 - 0.9 * fabs(D(pd2)) / sqrt(sqrt(D(sel.x * sel.x + sel.y * sel.y + sel.z * sel.z))));
    cf = make_float4(sw * pa, sw * pb, sw * pc, sw * pd2);
    ok = D(sw) > 0.1 ? 1 : 0;
  }
}

// jw: this lane's 27 words of LDS scratch for the 3x3 Jacobi
LOAM_D void mp_fit_query(const MpBuffers& b, int p, int q, int nsc, bool first, int4 n0, int4 n1, float4 sel,
                         float* jw, int& nfits, float4& cf, int& ok) {
  const bool corner = q < nsc;
  const int nfc = b.nfrom[p * 2 + 0];
  const float4* from = b.from + (size_t)p * b.map_cap + (corner ? 0 : nfc);
  MpFit* qfit = (MpFit*)b.q_fit + (size_t)p * b.cap_stack;
  ok = 0;
  cf = make_float4(0, 0, 0, 0);
  if (n1.x != 0x7fffffff && D(__int_as_float(n1.y)) < 1.0) {  // :719, :826
    MpFit f = qfit[q];
    if (first || f.n0.x != n0.x || f.n0.y != n0.y || f.n0.z != n0.z || f.n0.w != n0.w || f.n1.x != n1.x) {
      ++nfits;
      const int idx[5] = {n0.x, n0.y, n0.z, n0.w, n1.x};
      float4 nb[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        LOAM_CHECK(idx[k] >= 0 && idx[k] < (corner ? nfc : b.nfrom[p * 2 + 1]), idx[k], q);
        nb[k] = from[idx[k]];
      }
      f.n0 = n0;
      f.n1 = make_int4(n1.x, 0, 0, 0);
      mp_fit_compute(corner, nb, jw, f.g0, f.g1);
      qfit[q] = f;
    }
    mp_fit_residual(corner, f.g0, f.g1, sel, cf, ok);
  } else if (first) {
    // no fit this iteration: drop a fit left by an earlier frame (whose map indices name other
    // points) so that a later iteration cannot take it for this frame's
    qfit[q].n0 = make_int4(-1, -1, -1, -1);
  }
}

// sin / cos of the TobeMapped rotation for the rows
struct MpTrig {
  float srx, crx, sry, cry, srz, crz;
};
LOAM_D MpTrig mp_trig_of(const float* trig) { return {trig[0], trig[1], trig[2], trig[3], trig[4], trig[5]}; }
// the same values from the stored rotation (rot_store: dsin / dcos of the same TobeMapped angles),
// without the serial double sin / cos in the kernel prologue
LOAM_D MpTrig mp_trig_of(const loampose::MapRot& r) {
  return {(float)r.s0, (float)r.c0, (float)r.s1, (float)r.c1, (float)r.s2, (float)r.c2};
}

// The six values as one place in a loop sees them: the products of them that mp_row_jac forms
// are the same for every query, and the compiler would otherwise keep each in a vector register
// across the whole loop over the queries (k_mp_nnfit has none to spare); so they are formed
// where they are used
LOAM_D MpTrig mp_trig_here(MpTrig t) {
  asm volatile("" : "+v"(t.srx), "+v"(t.crx), "+v"(t.sry), "+v"(t.cry), "+v"(t.srz), "+v"(t.crz));
  return t;
}

// the accepted row's J (:897-921): a[0..5] and b = -coefficient.w
LOAM_D void mp_row_jac(const MpTrig& tg, float4 o, float4 c, float (&a)[6], float& bb) {
  const float srx = tg.srx, crx = tg.crx, sry = tg.sry, cry = tg.cry, srz = tg.srz, crz = tg.crz;
  a[0] = (crx * sry * srz * o.x + crx * crz * sry * o.y - srx * sry * o.z) * c.x +
         (-srx * srz * o.x - crz * srx * o.y - crx * o.z) * c.y +
         (crx * cry * srz * o.x + crx * cry * crz * o.y - cry * srx * o.z) * c.z;
  a[1] = ((cry * srx * srz - crz * sry) * o.x + (sry * srz + cry * crz * srx) * o.y + crx * cry * o.z) * c.x +
         ((-cry * crz - srx * sry * srz) * o.x + (cry * srz - crz * srx * sry) * o.y - crx * sry * o.z) * c.z;
  a[2] = ((crz * srx * sry - cry * srz) * o.x + (-cry * crz - srx * sry * srz) * o.y) * c.x +
         (crx * crz * o.x - crx * srz * o.y) * c.y +
         ((sry * srz + cry * crz * srx) * o.x + (crz * sry - cry * srx * srz) * o.y) * c.z;
  a[3] = c.x;
  a[4] = c.y;
  a[5] = c.z;
  bb = -c.w;
}

LOAM_D void mp_row_accum(const MpTrig& tg, float4 o, float4 c, double (&acc)[28]) {
  float a[6], bb;
  mp_row_jac(tg, o, c, a, bb);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int jj = i; jj < 6; ++jj) { acc[k] = loamla::dmac(acc[k], a[i], a[jj]); ++k; }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = loamla::dmac(acc[21 + i], a[i], bb);
  acc[27] += 1.0;
}

struct MpStepScratch {
  float lm_ws[loamla::kLmWs];
  int lm_iws[12];
  float AtA[36], AtB[6], X[6];
  float jE[6], jV[36];  // iteration 0: jacobi6_wave's eigen decomposition of AtA
};

// the first wave of the workgroup (the iteration-0 eigen decomposition, jacobi6_wave), the rest on
// lane 0: iteration bookkeeping, the 6x6 step when there are >= 50 rows (:886-889), the update (no
// NaN guard in mapping, :956-961) and the convergence test (:972)
LOAM_D void mp_step(const MpBuffers& b, int p, const double* tot, MpStepScratch& sh) {
  const int lane = lane_id();
  int* ist = b.istate + (size_t)p * kMpStateInts;
  float* st = b.state + (size_t)p * kMpStateFloats;
  const int iter = ist[kMiIters];
  const int nrows = (int)tot[27];
  // lane 0's global reads of the step, issued together up front (round trips on the serial chain)
  int c_rows = 0, degen = 0, c_deg = 0;
  float T[6] = {0, 0, 0, 0, 0, 0};
  if (lane == 0) {
    c_rows = ist[kMiRows];
    degen = ist[kMiDegen];
    c_deg = ist[kMiDegSteps];
#pragma unroll
    for (int q = 0; q < 6; ++q) T[q] = st[kMpTobe + q];
  }
  if (nrows >= 50 && lane == 0) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int jj = i; jj < 6; ++jj) {
        sh.AtA[i * 6 + jj] = (float)tot[k];
        sh.AtA[jj * 6 + i] = (float)tot[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) sh.AtB[i] = (float)tot[21 + i];
  }
  const bool solve = nrows >= 50;  // (uniform)
  bool eig = solve && iter == 0, cert = false;
  if (solve) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // lane 0's AtA / AtB, for the wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (eig) {
      cert = loamla::nondegenerate_certified(sh.AtA, 100.0f);  // every lane, the same answer
      eig = !cert;
      if (eig) loamla::jacobi6_wave(sh.AtA, sh.jE, sh.jV);
    }
    // the QR solve by the whole wave; lane 0 goes on with X
    loamla::lm_step_wave(sh.AtA, sh.AtB, iter, 100.0f, &degen, st + kMpMatP, sh.X, sh.lm_ws, sh.lm_iws,
                         eig ? sh.jE : nullptr, eig ? sh.jV : nullptr, cert);
  }
  if (lane != 0) return;
  ist[kMiIters] = iter + 1;
  ist[kMiRows] = c_rows + nrows;
  ist[kMiRowsLast] = nrows;
  if (solve) {
    ist[kMiDegen] = degen;
    if (degen) ist[kMiDegSteps] = c_deg + 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      T[q] = T[q] + sh.X[q];
      st[kMpTobe + q] = T[q];
    }
    rot_store(b, p, T);
    const float dR = loamla::delta_r(sh.X), dT = loamla::delta_t(sh.X);
    if (D(dR) < 0.05 && D(dT) < 0.05) ist[kMiStop] = 1;
  }
  if (iter + 1 >= b.max_iter) ist[kMiStop] = 1;
}
}  // namespace

// the fused step of one-wave workgroups (k_mp_nnfit<true>): the wave's row sums as
// this workgroup's partial (write-through), and the last workgroup of the instance to arrive sums
// the G partials in workgroup order and runs the step
// red: the wave's sums reduce-scattered (wave_reduce_scatter_28: lanes 2v, 2v+1 hold value v)
LOAM_D void mp_store_partial_and_step(const MpBuffers& b, int p, int wg, int G, double red) {
  static_assert(kMpFitThreads == 64, "one wave per workgroup: the wave's sums are the partial");
  const int lane = lane_id();
  if ((lane & 1) == 0 && (lane >> 1) < 28)
    store_partial(&b.part[((size_t)p * kMpFitGridMax + wg) * 28 + (lane >> 1)], red);
  __shared__ int sh_last;
  __shared__ double tot[28];
  __shared__ MpStepScratch sh;
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) sh_last = arrive_last(&b.done[p], G);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  {  // fixed order over the workgroups: lane (half h, value v) sums half h of the partials in
     // order, sixteen loads in flight per round, then the two halves are added in order
    const int v = lane % 28, h = lane / 28, G2 = (G + 1) / 2;
    const int g0 = h == 0 ? 0 : G2, g1 = h == 0 ? G2 : G;
    const double* pp = b.part + (size_t)p * kMpFitGridMax * 28 + v;
    double sum = 0.0;
    if (h < 2) {
      for (int g = g0; g < g1; g += 16) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          t[u] = g + u < g1 ? __hip_atomic_load(&pp[(size_t)(g + u) * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (g + u < g1) sum += t[u];
      }
    }
    const double upper = __shfl_down(sum, 28, 64);
    if (lane < 28) tot[lane] = sum + upper;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane == 0) b.done[p] = 0;
  mp_step(b, p, tot, sh);
}
// One mapping L-M iteration's correspondences in one launch: lane per query, the 5-NN search
// (knn5_flat, seeded) then the fit and row — the fit needs only the lane's own five neighbours —
// in one-wave workgroups whose 27-entry candidate lists and 27-word Jacobi scratch share one LDS
// array (the wave's search is over before its fits begin).  Rows in query order per workgroup.
// FUSED: the workgroup's partial + the last workgroup's step (mp_store_partial_and_step); else the
// rows go to q_ok / q_cf for k_mp_iter.  COUNT: the work counters.
#ifndef LOAM_NNFIT_WPE
#define LOAM_NNFIT_WPE 4
#endif
template <bool FUSED, bool COUNT>
__global__ __launch_bounds__(kMpFitThreads) __attribute__((amdgpu_waves_per_eu(LOAM_NNFIT_WPE))) void k_mp_nnfit(MpBuffers b) {
  constexpr int NT = kMpFitThreads;
  static_assert(NT == 64, "the list / scratch sharing needs one wave per workgroup");
  const XcdBlock blk = xcd_block();
  const int p = blk.y, tid = threadIdx.x;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  const bool first = ist[kMiIters] == 0;
  __shared__ uint32_t lds[kNnListCap * NT];  // candidate lists (column tid, stride NT) / Jacobi rows
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const loampose::MapRot r = rot_load(b, p);
  const MpNnCtx c = mp_nn_ctx(b, p);
  const MpTrig tg0 = mp_trig_of(r);
  float* jw = (float*)lds + tid * 27;
  int nfits = 0, work = 0;
  // FUSED: the rows of each pass over the queries are reduce-scattered over the wave at once (no
  // 28 fp64 sums live across the search), the passes' sums added in pass order (one pass per lane
  // for a VLP-16 stack)
  double red = 0.0;
  // FUSED: lane 2t's term t of the 28 sums (JᵀJ upper triangle row-major, Jᵀb, rows) as the
  // product of row entries term_x * term_y (mp_row_accum's order; entry 7 = 1 per accepted row)
  int term_x = -1, term_y = -1;
  if (FUSED && (tid & 1) == 0 && (tid >> 1) < 28) {
    const int t = tid >> 1;
    if (t < 21) {
      int i = 0, r0 = t;
      while (r0 >= 6 - i) { r0 -= 6 - i; ++i; }
      term_x = i;
      term_y = i + r0;
    } else if (t < 27) {
      term_x = t - 21;
      term_y = 6;
    } else {
      term_x = 7;
      term_y = 7;
    }
  }
  // one record per query (MpFit in q_fit): the 5-NN of the last iteration (i0..i3 | i4, 0,
  // distinct, fit valid) and the fit made for them — the seeds and the reuse test in one read
  MpFit* qrec = (MpFit*)b.q_fit + (size_t)p * b.cap_stack;
  for (int q0 = blk.x * NT; q0 < nq; q0 += gridDim.x * NT) {  // (wave-uniform trip count)
    const int q = q0 + tid;
    const bool corner = q < nsc;
    float4 sel = make_float4(0, 0, 0, 0), o = sel, cf = sel;
    int4 r0 = make_int4(-1, -1, -1, -1), r1 = make_int4(0, 0, 0, 0);
    bool row_ok = false;
    Top5 t;
    if (q < nq) {
      o = c.stack[corner ? q : b.capC + (q - nsc)];
      if (!first) { r0 = qrec[q].n0; r1 = qrec[q].n1; }
      sel = loampose::point_to_map(r, o);
      mp_nn_seed_from(c, q, corner, first, r0, r1, sel, t, work);
#ifdef LOAM_DIAG_OVERFLOW  // (diagnostic build: the queries that overflowed their pending list, in mp_fits >> 20)
      int dg = 0;
      int* const diag = &dg;
#else
      int* const diag = nullptr;
#endif
      if (corner) knn5_flat<NT, 1, kNnListCap>(c.hcs, c.hcr, c.hcp, c.TC, sel, t, lds + tid, work, 0, diag);
      else knn5_flat<NT, 1, kNnListCap>(c.hss, c.hsr, c.hsp, c.TS, sel, t, lds + tid, work, 0, diag);
#ifdef LOAM_DIAG_OVERFLOW
      if (dg & kNnDiagOverflow) nfits += 1 << 20;
#endif
#ifdef LOAM_DIAG_SEARCH2  // (diagnostic build: the search twice, its cost measured by the difference)
      {
        Top5 t2;
        int w2 = 0;
        asm volatile("" ::: "memory");
        mp_nn_seed_from(c, q, corner, first, r0, r1, sel, t2, w2);
        if (corner) knn5_flat<NT, 1, kNnListCap>(c.hcs, c.hcr, c.hcp, c.TC, sel, t2, lds + tid, w2, 0);
        else knn5_flat<NT, 1, kNnListCap>(c.hss, c.hsr, c.hsp, c.TS, sel, t2, lds + tid, w2, 0);
        if (t2.i(0) != t.i(0)) nfits += 1 << 20;
      }
#endif
      LOAM_CHECK(q < b.cap_stack && (t.i(4) == 0x7fffffff || t.i(4) < (corner ? c.nfc : c.nfs)), q, t.i(4));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // every lane's list reads are done before the scratch reuse
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (q < nq) {
      const int4 n0 = make_int4(t.i(0), t.i(1), t.i(2), t.i(3));
      // the stored fit is this list's when the list is unchanged and the fit was made (a fit is
      // a function of the five map points alone: reusing it is bit-identical to refitting)
      bool valid = !first && r1.w && r0.x == n0.x && r0.y == n0.y && r0.z == n0.z && r0.w == n0.w &&
                   r1.x == t.i(4);
      int ok = 0;
      if (t.i(4) != 0x7fffffff && D(t.d(4)) < 1.0) {  // :719, :826
        float4 g0, g1;
        if (valid) {
          g0 = qrec[q].g0;
          g1 = qrec[q].g1;
        } else {
          ++nfits;
          const float4* from = corner ? c.fromC : c.fromS;
          float4 nb[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            LOAM_CHECK(t.i(k) >= 0 && t.i(k) < (corner ? c.nfc : c.nfs), t.i(k), q);
            nb[k] = from[t.i(k)];
          }
          mp_fit_compute(corner, nb, jw, g0, g1);
#ifdef LOAM_DIAG_FIT2  // (diagnostic build: every fit twice)
          {
            float4 h0, h1;
            asm volatile("" ::: "memory");
            mp_fit_compute(corner, nb, jw, h0, h1);
            if (h0.x != g0.x) nfits += 1 << 20;
          }
#endif
          qrec[q].g0 = g0;
          qrec[q].g1 = g1;
          valid = true;
        }
        mp_fit_residual(corner, g0, g1, sel, cf, ok);
      }
      // the record is written only when it changes: a reused fit's list is the stored one (the
      // next iteration's seeds and reuse test read indices and flags only)
      const int4 n1 = make_int4(t.i(4), 0, top5_distinct(t), valid ? 1 : 0);
      if (first || r0.x != n0.x || r0.y != n0.y || r0.z != n0.z || r0.w != n0.w || r1.x != n1.x || r1.z != n1.z ||
          r1.w != n1.w) {
        qrec[q].n0 = n0;
        qrec[q].n1 = n1;
      }
      if constexpr (!FUSED) {  // (k_mp_iter reads the rows back; the fused step sums them below)
        qok[q] = (int8_t)ok;
        qcf[q] = cf;
      }
      row_ok = ok != 0;
    }
    if constexpr (FUSED) {  // (outside the branch: every lane takes part)
      // the pass's rows through LDS (8 floats per lane: J, b, 1 when accepted, else zeros), then
      // lane 2t sums term t over the wave's rows in query order: no 28 fp64 sums per lane
      float a6[6] = {0, 0, 0, 0, 0, 0}, bb = 0.0f;
      const MpTrig tg = mp_trig_here(tg0);
      if (row_ok) mp_row_jac(tg, o, cf, a6, bb);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();  // the fits' scratch reads are done
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      float* rw = (float*)lds + tid * 8;
#pragma unroll
      for (int k = 0; k < 6; ++k) rw[k] = a6[k];
      rw[6] = bb;
      rw[7] = row_ok ? 1.0f : 0.0f;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (term_x >= 0) {
        const float* rows = (const float*)lds;
        double s = 0.0;
#pragma unroll 16
        for (int l = 0; l < NT; ++l) s = loamla::dmac(s, rows[l * 8 + term_x], rows[l * 8 + term_y]);
        red += s;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // the fits' scratch is free before the next lists
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  nfits = wave_sum(nfits);
  if (lane_id() == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  if (COUNT) {
    const int ncand = wave_sum(work & ((1 << kWorkCellShift) - 1)), ncell = wave_sum(work >> kWorkCellShift);
    if (lane_id() == 0 && ncand) {
      atomicAdd(&ist[kMiNnCand], ncand);
      atomicAdd(&ist[kMiNnCells], ncell);
    }
  }
  if constexpr (FUSED) mp_store_partial_and_step(b, p, blk.x, (int)gridDim.x, red);
}

namespace {
struct MpIterShared {
  double red[16][28];  // (up to 1024 threads)
  double tot[28];
  float trig[6];
  MpStepScratch step;
};
}  // namespace

// the normal equations of the accepted rows (:879-974) and the 6x6 step, one workgroup per
// instance; rows = the accepted correspondences of this iteration, in stack order
// NT threads per instance: 256 for large batches, 1024 for small ones (a shorter row chain per lane)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_iter(MpBuffers b) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  __shared__ MpIterShared sh;
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  const int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  const float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const MpTrig tg = mp_trig_of(rot_load(b, p));
  const float srx = tg.srx, crx = tg.crx, sry = tg.sry, cry = tg.cry, srz = tg.srz, crz = tg.crz;
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  // four rows' loads in flight per step; the rows are still summed in the lane's q order
  for (int q0 = tid; q0 < nq; q0 += 4 * NT) {  // :897-921
    int8_t okv[4];
    float4 ov[4], cv4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * NT;
      okv[u] = q < nq ? qok[q] : (int8_t)0;
      ov[u] = q < nq ? stack[q < nsc ? q : b.capC + (q - nsc)] : make_float4(0, 0, 0, 0);
      cv4[u] = q < nq ? qcf[q] : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
    if (!okv[u]) continue;
    const float4 o = ov[u], c = cv4[u];
    float a[6];
    a[0] = (crx * sry * srz * o.x + crx * crz * sry * o.y - srx * sry * o.z) * c.x +
           (-srx * srz * o.x - crz * srx * o.y - crx * o.z) * c.y +
           (crx * cry * srz * o.x + crx * cry * crz * o.y - cry * srx * o.z) * c.z;
    a[1] = ((cry * srx * srz - crz * sry) * o.x + (sry * srz + cry * crz * srx) * o.y + crx * cry * o.z) * c.x +
           ((-cry * crz - srx * sry * srz) * o.x + (cry * srz - crz * srx * sry) * o.y - crx * sry * o.z) * c.z;
    a[2] = ((crz * srx * sry - cry * srz) * o.x + (-cry * crz - srx * sry * srz) * o.y) * c.x +
           (crx * crz * o.x - crx * srz * o.y) * c.y +
           ((sry * srz + cry * crz * srx) * o.x + (crz * sry - cry * srx * srz) * o.y) * c.z;
    a[3] = c.x;
    a[4] = c.y;
    a[5] = c.z;
    const float bb = -c.w;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = i; jj < 6; ++jj) acc[k++] += (double)a[i] * (double)a[jj];  // (dmac measured slower here)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += (double)a[i] * (double)bb;
    acc[27] += 1.0;
  }
  }
  wave_reduce_scatter_28(acc);  // lanes 2v, 2v+1: the wave sum of value v
  if ((lane & 1) == 0 && (lane >> 1) < 28) sh.red[w][lane >> 1] = acc[0];
  __syncthreads();
  if (tid < 28) {
    double v = sh.red[0][tid];
    for (int ww = 1; ww < NT / 64; ++ww) v += sh.red[ww][tid];
    sh.tot[tid] = v;
  }
  __syncthreads();
  if (tid < 64) mp_step(b, p, sh.tot, sh.step);  // the first wave
}

// Small batches (streaming, config 2): the whole iteration in one launch — each lane its query's
// 5-NN, fit and row, fp64 partials per workgroup, and the last workgroup of the instance to finish
// sums them in a fixed order and runs the step (three launches and a one-workgroup row pass fewer
// per iteration).
__global__ __launch_bounds__(kMpQueryThreads) void k_mp_lm_small(MpBuffers b) {
  const int p = blockIdx.y, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  LOAM_PH(const unsigned long long ph0 = ph_now(); if (tid == 0) ph_start(&g_ph_mp, ph0);)
  __shared__ uint32_t lists[27 * kMpQueryThreads];
  __shared__ float jac[kMpQueryThreads][27];
  __shared__ double red[kMpQueryThreads / 64][28];
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const bool first = ist[kMiIters] == 0;
  const loampose::MapRot r = rot_load(b, p);
  const MpNnCtx c = mp_nn_ctx(b, p);
  int work = 0, nfits = 0;  // (work: the batch kernel's profiling counter; not summed here)
  const MpTrig tg = mp_trig_of(r);
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  // each lane's row is added right after its fit (same queries, same order per lane as a
  // separate pass over the stored rows: identical sums, one reload round trip fewer)
  // kMpNnLanes lanes per query: the 5-NN search split over the group, the fit and row on its first lane
  constexpr int L = kMpNnLanes, QPB = kMpQueryThreads / L;
  const int sub = tid % L;
  for (int q = blockIdx.x * QPB + tid / L; q < nq; q += gridDim.x * QPB) {
    LOAM_PH(const unsigned long long pq0 = ph_now();)
    float4 sel;
    Top5 t;
    mp_nn_query<kMpQueryThreads, L>(b, c, q, nsc, first, r, lists + tid, sel, t, work, sub);
    LOAM_PH(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long pq1 = ph_now();)
    float4 cf = make_float4(0, 0, 0, 0);
    int ok = 0;
    if (sub == 0) {
      mp_fit_query(b, p, q, nsc, first, make_int4(t.i(0), t.i(1), t.i(2), t.i(3)),
                   make_int4(t.i(4), __float_as_int(t.d(4)), 0, 0), sel, jac[tid], nfits, cf, ok);
      qok[q] = (int8_t)ok;
      qcf[q] = cf;
      if (ok) mp_row_accum(tg, stack[q < nsc ? q : b.capC + (q - nsc)], cf, acc);
    }
    LOAM_PH(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long pq2 = ph_now();
            if (lane == 0) ph_query(&g_ph_mp, first ? 0 : 1, pq1 - pq0, pq2 - pq1);)
  }
  nfits = wave_sum(nfits);
  if (lane == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  wave_reduce_scatter_28(acc);
  if ((lane & 1) == 0 && (lane >> 1) < 28) red[w][lane >> 1] = acc[0];
  __syncthreads();
  const int G = (int)gridDim.x;
  if (tid < 28) {
    double v = red[0][tid];
    for (int ww = 1; ww < kMpQueryThreads / 64; ++ww) v += red[ww][tid];
    store_partial(&b.part[((size_t)p * kMpSmallGrid + blockIdx.x) * 28 + tid], v);
  }
  __shared__ int sh_last;
  __shared__ double slice[8][28];
  __shared__ double tot[28];
  __shared__ MpStepScratch sh;
  __syncthreads();
  LOAM_PH(const int phk = first ? 0 : 1; const unsigned long long ph1 = ph_now();
          if (tid == 0) ph_arrive(&g_ph_mp, phk, ph0, ph1);)
  // (store_partial / arrive_last: the partials are drained write-through before the counter add;
  // the last workgroup acquires at agent scope, then reads them with sc1 loads)
  if (tid == 0)
    sh_last = arrive_last(&b.done[p], G);
  __syncthreads();
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  LOAM_PH(const unsigned long long ph2 = ph_now();)
  if (tid < 8 * 28) {  // fixed-order sum: slice s holds partials s, s + 8, ... (all in flight)
    const int v = tid % 28, sl = tid / 28;
    const double* pp = b.part + (size_t)p * kMpSmallGrid * 28 + v;
    double t8[kMpSmallGrid / 8];
#pragma unroll
    for (int u = 0; u < kMpSmallGrid / 8; ++u) {
      const int g = sl + 8 * u;
      t8[u] = g < G ? __hip_atomic_load(&pp[(size_t)g * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
    double a1 = 0.0;
#pragma unroll
    for (int u = 0; u < kMpSmallGrid / 8; ++u)
      if (sl + 8 * u < G) a1 += t8[u];
    slice[sl][v] = a1;
  }
  __syncthreads();
  if (tid < 28) {
    double v = slice[0][tid];
#pragma unroll
    for (int sl = 1; sl < 8; ++sl) v += slice[sl][tid];
    tot[tid] = v;
  }
  __syncthreads();
  LOAM_PH(const unsigned long long ph3 = ph_now();)
  if (tid < 64) {  // the first wave
    if (tid == 0) b.done[p] = 0;
    mp_step(b, p, tot, sh);
    LOAM_PH(const unsigned long long ph4 = ph_now(); if (tid == 0) ph_last(&g_ph_mp, phk, ph1, ph2, ph3, ph4);)
  }
}

// ---- the one-instance mapping L-M as one persistent launch (streaming: config 3, config 2) ----
// k_mp_lm_small's iteration (5-NN, fit, row per query group of kMpNnLanes lanes) for every
// iteration in one launch, as k_od_lm_stream does for the odometry: a query stays on the same
// lanes for the whole loop (its 5-NN seeds and fit record are read back by the lanes that wrote
// them), the partial sums are exchanged per iteration with write-through stores and a publication
// word per workgroup, and every workgroup sums all G partials in workgroup order and runs the step
// on its own copy of the state: the same transform and the same convergence decision everywhere.
struct MpLsState {
  float T[6], matP[36];
  int degen, iters, rows, deg_steps, stop;
};

// mp_step on the workgroup-local state (the first wave): the same arithmetic and decisions
LOAM_D void mp_step_ls(int max_iter, const double* tot, MpLsState& S, MpStepScratch& sh) {
  const int lane = lane_id();
  const int iter = S.iters;
  const int nrows = (int)tot[27];
  if (nrows >= 50 && lane == 0) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int jj = i; jj < 6; ++jj) {
        sh.AtA[i * 6 + jj] = (float)tot[k];
        sh.AtA[jj * 6 + i] = (float)tot[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) sh.AtB[i] = (float)tot[21 + i];
  }
  const bool solve = nrows >= 50;  // (uniform)
  bool eig = solve && iter == 0, cert = false;
  int degen = S.degen;
  if (solve) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (eig) {
      cert = loamla::nondegenerate_certified(sh.AtA, 100.0f);
      eig = !cert;
      if (eig) loamla::jacobi6_wave(sh.AtA, sh.jE, sh.jV);
    }
    loamla::lm_step_wave(sh.AtA, sh.AtB, iter, 100.0f, &degen, S.matP, sh.X, sh.lm_ws, sh.lm_iws,
                         eig ? sh.jE : nullptr, eig ? sh.jV : nullptr, cert);
  }
  if (lane != 0) return;
  S.iters = iter + 1;
  S.rows += nrows;
  if (solve) {
    S.degen = degen;
    if (degen) ++S.deg_steps;
#pragma unroll
    for (int q = 0; q < 6; ++q) S.T[q] = S.T[q] + sh.X[q];
    const float dR = loamla::delta_r(sh.X), dT = loamla::delta_t(sh.X);
    if (D(dR) < 0.05 && D(dT) < 0.05) S.stop = 1;
  }
  if (iter + 1 >= max_iter) S.stop = 1;
}

__global__ __launch_bounds__(kMpQueryThreads) void k_mp_lm_stream(MpBuffers b) {
  const int g = blockIdx.x, G = gridDim.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6, p = 0;
  int* ist = b.istate;
  float* st = b.state;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;  // (the same value in every workgroup)
  __shared__ uint32_t lists[27 * kMpQueryThreads];
  __shared__ float jac[kMpQueryThreads][27];
  __shared__ double red[kMpQueryThreads / 64][28], slice[8][28], tot[28];
  __shared__ MpStepScratch sh;
  __shared__ MpLsState S;
  __shared__ unsigned long long sh_epoch;
  if (tid < 6) S.T[tid] = st[kMpTobe + tid];
  if (tid < 36) S.matP[tid] = st[kMpMatP + tid];
  if (tid == 0) {
    S.degen = ist[kMiDegen];
    S.iters = ist[kMiIters];
    S.rows = ist[kMiRows];
    S.deg_steps = ist[kMiDegSteps];
    S.stop = 0;
    sh_epoch = b.ls_epoch[0];
  }
  __syncthreads();
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack;
  int8_t* qok = b.q_ok;
  float4* qcf = b.q_cf;
  const MpNnCtx c = mp_nn_ctx(b, p);
  constexpr int L = kMpNnLanes, QPB = kMpQueryThreads / L;
  const int sub = tid % L;
  const unsigned long long tag0 = sh_epoch << 16;  // (iterations + 1 <= 1001 < 2^16: loam_create bounds max_iter)
  int nfits = 0;
  for (int it = 0; it < b.max_iter; ++it) {
    const bool first = S.iters == 0;
    const loampose::MapRot r = loampose::map_rot(S.T);  // (rot_store's values: the same dsin / dcos)
    const MpTrig tg = mp_trig_of(r);
    int work = 0;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for (int q = g * QPB + tid / L; q < nq; q += G * QPB) {
      float4 sel;
      Top5 t;
      mp_nn_query<kMpQueryThreads, L>(b, c, q, nsc, first, r, lists + tid, sel, t, work, sub);
      float4 cf = make_float4(0, 0, 0, 0);
      int ok = 0;
      if (sub == 0) {
        mp_fit_query(b, p, q, nsc, first, make_int4(t.i(0), t.i(1), t.i(2), t.i(3)),
                     make_int4(t.i(4), __float_as_int(t.d(4)), 0, 0), sel, jac[tid], nfits, cf, ok);
        qok[q] = (int8_t)ok;
        qcf[q] = cf;
        if (ok) mp_row_accum(tg, stack[q < nsc ? q : b.capC + (q - nsc)], cf, acc);
      }
    }
    wave_reduce_scatter_28(acc);
    if ((lane & 1) == 0 && (lane >> 1) < 28) red[w][lane >> 1] = acc[0];
    __syncthreads();
    const int par = it & 1;
    if (tid < 28) {  // this workgroup's partial, waves in order, stored write-through
      double v = red[0][tid];
      for (int ww = 1; ww < kMpQueryThreads / 64; ++ww) v += red[ww][tid];
      store_partial(&b.ls_part[((size_t)par * kMpSmallGrid + g) * 28 + tid], v);
    }
    if (tid < 64) {
      __builtin_amdgcn_wave_barrier();  // (every lane's store drained: store_partial waits for it)
      if (tid == 0)
        __hip_atomic_store(&b.ls_flag[g], tag0 + (unsigned long long)(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < G) {  // every workgroup's partial of this iteration
      const unsigned long long want = tag0 + (unsigned long long)(it + 1);
      while (__hip_atomic_load(&b.ls_flag[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want)
        __builtin_amdgcn_s_sleep(1);
    }
    __syncthreads();
    if (tid < 8 * 28) {  // fixed order: slice s sums partials s, s + 8, ...; the slices in order
      const int v = tid % 28, sl = tid / 28;
      const double* pp = b.ls_part + (size_t)par * kMpSmallGrid * 28 + v;
      double t8[kMpSmallGrid / 8];
#pragma unroll
      for (int u = 0; u < kMpSmallGrid / 8; ++u) {
        const int gg = sl + 8 * u;
        t8[u] = gg < G ? __hip_atomic_load(&pp[(size_t)gg * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
      double a1 = 0.0;
#pragma unroll
      for (int u = 0; u < kMpSmallGrid / 8; ++u)
        if (sl + 8 * u < G) a1 += t8[u];
      slice[sl][v] = a1;
    }
    __syncthreads();
    if (tid < 28) {
      double v = slice[0][tid];
#pragma unroll
      for (int sl = 1; sl < 8; ++sl) v += slice[sl][tid];
      tot[tid] = v;
    }
    __syncthreads();
    if (tid < 64) mp_step_ls(b.max_iter, tot, S, sh);
    __syncthreads();
    if (S.stop) break;
  }
  nfits = wave_sum(nfits);
  if (lane == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  if (g == 0) {  // the state for the kernels after the loop (the same in every workgroup)
    if (tid < 6) st[kMpTobe + tid] = S.T[tid];
    if (tid < 36) st[kMpMatP + tid] = S.matP[tid];
    if (tid == 0) {
      rot_store(b, p, S.T);
      ist[kMiDegen] = S.degen;
      ist[kMiIters] = S.iters;
      ist[kMiRows] = S.rows;
      ist[kMiDegSteps] = S.deg_steps;
      ist[kMiStop] = S.stop;
    }
  }
}

// workgroups of k_mp_lm_stream (kMpSmallGrid, as k_mp_lm_small), or 0 when they could not all be
// resident at once (the per-iteration launches run instead)
int mp_lm_stream_grid() {
  static int cap[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cap[dev] == 0) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_mp_lm_stream, kMpQueryThreads, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      per_cu = cus = 0;
    cap[dev] = std::max(1, per_cu * cus);
  }
  // (a margin of 2: other streams' kernels may hold slots a while; half the grid loops twice)
  return 2 * kMpSmallGrid <= cap[dev] ? kMpSmallGrid : (kMpSmallGrid <= cap[dev] ? kMpSmallGrid / 2 : 0);
}

// transformUpdate (:199-232) for the instances whose L-M ran; the IMU blend (:224-225) when the
// host found IMU data for the odometry stamp
__global__ void k_mp_lm_end(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; b.vg.counts[2] = 0; b.vg.counts[3] = 0; }  // (vg_cubes' lists)
  if (p >= b.P) return;
  const int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan]) return;
  float* st = b.state + (size_t)p * kMpStateFloats;
  if (ist[kMiImu]) {
    const float imuRollLast = st[kMpImuRP], imuPitchLast = st[kMpImuRP + 1];
    st[kMpTobe + 0] = (float)(0.998 * D(st[kMpTobe + 0]) + 0.002 * D(imuPitchLast));
    st[kMpTobe + 2] = (float)(0.998 * D(st[kMpTobe + 2]) + 0.002 * D(imuRollLast));
    rot_store(b, p, st + kMpTobe);
  }
  for (int k = 0; k < 6; ++k) {
    st[kMpBef + k] = st[kMpSum + k];
    st[kMpAft + k] = st[kMpTobe + k];
  }
}

namespace {

// ---------------------------------------------------------------- insertion (:980-1016)
// one workgroup per instance: cube slot of every stack point (corner, then surf), stable ranks by
// one wave walking the stack in order, per-cube prefix, scatter of the map-frame points.
// (k_cm_rank below restates the slot and ranking statements for loam_lanes_map_commit, whose n = 1
// result must equal this kernel's bit for bit: a change to either belongs in both.)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_insert(MpBuffers b, int* slot_of, int* rank_of) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  const int* ist = b.istate + (size_t)p * kMpStateInts;
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  const loampose::MapRot r = rot_load(b, p);
  const int cW = ist[kMiCenW], cH = ist[kMiCenH], cD = ist[kMiCenD];
  int* so = slot_of + (size_t)p * b.cap_stack;
  int* ro = rank_of + (size_t)p * b.cap_stack;
  __shared__ int cnt[2][kCubeNum];
  __shared__ int scratch[NT / 64 + 1];
  // the (slot, kind) keys the stack uses, as a bitmap; their dense numbering (prefix popcounts)
  // lets every wave keep its own counts when few keys occur (the usual case: a sweep touches a
  // few dozen cubes)
  constexpr int kKeyWords = (2 * kCubeNum + 31) / 32, kDense = 512, kWaves = NT / 64;
  __shared__ unsigned keybits[kKeyWords];
  __shared__ int keypre[kKeyWords + 1];
  __shared__ int wcnt[kWaves][kDense];
  for (int i = tid; i < 2 * kCubeNum; i += NT) cnt[i / kCubeNum][i % kCubeNum] = 0;
  for (int i = tid; i < kKeyWords; i += NT) keybits[i] = 0u;
  for (int i = tid; i < kWaves * kDense; i += NT) wcnt[i / kDense][i % kDense] = 0;
  __syncthreads();
  const int nst = nsc + nss;
  for (int q = tid; q < nst; q += NT) {
    const float4 a = loampose::point_to_map(r, stack[q < nsc ? q : b.capC + (q - nsc)]);
    const int ci = cube_of(a.x, cW), cj = cube_of(a.y, cH), ck = cube_of(a.z, cD);
    const bool in = ci >= 0 && ci < kCubeW && cj >= 0 && cj < kCubeH && ck >= 0 && ck < kCubeD;
    const int s = in ? cube_index(ci, cj, ck) : -1;
    so[q] = s;
    if (s >= 0) {
      const int key = s * 2 + (q < nsc ? 0 : 1);
      atomicOr(&keybits[key >> 5], 1u << (key & 31));
    }
  }
  __threadfence_block();
  __syncthreads();
  {  // exclusive prefix of the words' popcounts
    constexpr int kPer = (kKeyWords + NT - 1) / NT;
    int sum = 0;
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kKeyWords) sum += __popc(keybits[i]);
    }
    int tot;
    int run = block_excl_scan<NT>(sum, scratch, tot);
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kKeyWords) {
        keypre[i] = run;
        run += __popc(keybits[i]);
      }
    }
    if (tid == 0) keypre[kKeyWords] = tot;
  }
  __syncthreads();
  const int nkeys = keypre[kKeyWords];
  if (nkeys <= kDense) {
    // stable ranks, all waves: wave w ranks its contiguous chunk of the stack (in order, per dense
    // key), then each key's chunk counts are prefixed in wave order
    const int w = tid >> 6, chunk = ((nst + kWaves * 64 - 1) / (kWaves * 64)) * 64;
    const int q0 = w * chunk, q1 = min(nst, q0 + chunk);
    constexpr int kAhead = 8;  // slot loads of eight 64-point steps in flight (the walk is load-latency bound)
    int sa[kAhead];
    for (int base = q0; base < q1; base += 64) {
      const int step = ((base - q0) >> 6) % kAhead;
      if (step == 0) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int qq = base + u * 64 + lane;
          sa[u] = qq < q1 ? so[qq] : -1;
        }
      }
      const int q = base + lane;
      const bool v = q < q1;
      int s = -1;
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (u == step) s = sa[u];
      const int key = s < 0 ? -1 : s * 2 + (q < nsc ? 0 : 1);
      const int id = key < 0 ? -1 : keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      uint64_t m = __ballot(v && id >= 0);
      int rank = 0;
      while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int il = __builtin_amdgcn_readlane(id, leader);
        const uint64_t mm = __ballot(v && id == il);
        const int basecnt = wcnt[w][il];
        if (v && id == il) rank = basecnt + __popcll(mm & lanemask_lt());
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) wcnt[w][il] = basecnt + __popcll(mm);
        __builtin_amdgcn_wave_barrier();
        m &= ~mm;
      }
      if (v) ro[q] = rank;
    }
    __threadfence_block();
    __syncthreads();
    // per dense key: chunk bases in wave order (wcnt becomes the base), total into cnt
    for (int i = tid; i < 2 * kCubeNum; i += NT) {
      if (!(keybits[i >> 5] & (1u << (i & 31)))) continue;
      const int id = keypre[i >> 5] + __popc(keybits[i >> 5] & ((1u << (i & 31)) - 1u));
      int run = 0;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) {
        const int c = wcnt[ww][id];
        wcnt[ww][id] = run;
        run += c;
      }
      cnt[i & 1][i >> 1] = run;
    }
    __threadfence_block();
    __syncthreads();
    for (int q = tid; q < nst; q += NT) {
      const int s = so[q];
      if (s < 0) continue;
      const int key = s * 2 + (q < nsc ? 0 : 1);
      const int id = keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      ro[q] += wcnt[q / chunk][id];
    }
  } else if (tid < 64) {  // many keys: stable ranks by one wave, stack order
    for (int base = 0; base < nsc + nss; base += 64) {
      const int q = base + lane;
      const bool v = q < nsc + nss;
      const int kind = q < nsc ? 0 : 1;
      const int s = v ? so[q] : -1;
      const int key = s < 0 ? -1 : s * 2 + kind;
      uint64_t m = __ballot(v && key >= 0);
      int rank = 0;
      while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int kl = __builtin_amdgcn_readlane(key, leader);
        const uint64_t mm = __ballot(v && key == kl);
        const int basecnt = cnt[kl & 1][kl >> 1];
        if (v && key == kl) rank = basecnt + __popcll(mm & lanemask_lt());
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) cnt[kl & 1][kl >> 1] = basecnt + __popcll(mm);
        __builtin_amdgcn_wave_barrier();
        m &= ~mm;
      }
      if (v) ro[q] = rank;
    }
  }
  __syncthreads();
  // exclusive prefix over (kind, cube slot), kind-major: each thread owns a contiguous run of the
  // flattened counts (one block scan instead of one per 256 slots); offsets replace the counts in LDS
  int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  {
    constexpr int kFlat = 2 * kCubeNum, kPer = (kFlat + NT - 1) / NT;
    int* cf = &cnt[0][0];
    int sum = 0;
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kFlat) sum += cf[i];
    }
    int tot;
    int run = block_excl_scan<NT>(sum, scratch, tot);
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kFlat) {
        const int c = cf[i];
        cf[i] = run;
        run += c;
      }
    }
    __syncthreads();
    for (int i = tid; i < kFlat; i += NT) {
      const int kind = i / kCubeNum, s = i % kCubeNum;
      const int o = cf[i], nx = i + 1 < kFlat ? cf[i + 1] : tot;
      ac[s * 2 + kind] = nx - o;
      ao[s * 2 + kind] = o;
    }
  }
  __threadfence_block();
  __syncthreads();
  float4* app = b.app + (size_t)p * b.cap_stack;
  for (int q = tid; q < nsc + nss; q += NT) {
    const int s = so[q];
    if (s < 0) continue;
    const int kind = q < nsc ? 0 : 1;
    app[ao[s * 2 + kind] + ro[q]] = loampose::point_to_map(r, stack[q < nsc ? q : b.capC + (q - nsc)]);
  }
}

// per valid cube: DS input = old cube content ++ appended points (corner region, then surf region);
// thread per (kind, valid cube) segment, one block scan for the offsets
__global__ __launch_bounds__(kMpThreads) void k_mp_vseg(MpBuffers b) {
  static_assert(2 * kMaxValid <= kMpThreads, "one thread per segment");
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* slots = slot_table(b, b.pool_cur, p);
  const int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  __shared__ int scratch[16];
  const int kind = tid / kMaxValid, v = tid % kMaxValid;
  int n = 0, nold = 0;
  if (tid < 2 * kMaxValid && v < nv) {
    const int ind = b.valid[(size_t)p * kMaxValid + v];
    nold = slots[ind * 4 + 1 + 2 * kind];
    n = nold + ac[ind * 2 + kind];
  }
  int tot;
  const int ex = block_excl_scan<kMpThreads>(n, scratch, tot);
  const int lim = b.map_cap;
  if (tid < 2 * kMaxValid) {
    // the reference order fills segments in (kind, v) order; a segment that would pass the
    // capacity is emptied and flags the instance (as the sequential walk did)
    const bool over = ex + n > lim;
    const int sidx = p * 2 * kMaxValid + tid;
    const int base = (int)((size_t)p * b.map_cap) + (over ? 0 : ex);
    b.vseg_b[sidx] = base;
    b.vseg_e[sidx] = base + (over ? 0 : n);
    b.vseg_leaf[sidx] = kind == 0 ? 0.2f : 0.4f;
    if (over && n > 0) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_MAP;
    b.vseg_nold[sidx] = nold;
    b.vseg_skip[sidx] = 0;
    if (over || n == 0) {
      b.vseg_cnt[sidx] = 0;  // (not in the VoxelGrid's list)
    } else {
      b.vg_lin[atomicAdd(b.vg.counts + 2, 1)] = sidx;
      // long segments with a short appended tail: the incremental VoxelGrid may take them
      if (b.tune.vg_merge && vg_merge_eligible(n, nold, b.tune.vg_merge_min))
        b.vg_mlist[atomicAdd(b.vg.counts + 3, 1)] = sidx;
    }
  }
}

// the DS input of every valid-cube segment, flattened over the instance's points: the segments
// are contiguous in (kind, valid cube) order, so a point finds its segment by binary search over
// their starts (LDS) and copies from the old pool or the appended stack points
__global__ __launch_bounds__(256) void k_mp_vcopy(MpBuffers b) {
  constexpr int NS = 2 * kMaxValid;
  const int p = blockIdx.y, tid = threadIdx.x;
  if (b.istate[(size_t)p * kMpStateInts + kMiErr] & ERR_CAP_MAP) return;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* slots = slot_table(b, b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  const int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  const float4* app = b.app + (size_t)p * b.cap_stack;
  __shared__ int sb[NS + 1], snold[NS], soff[NS], sapp[NS];
  const int base = (int)((size_t)p * b.map_cap);
  if (tid < NS) {
    const int kind = tid / kMaxValid, v = tid % kMaxValid;
    sb[tid] = b.vseg_b[p * NS + tid] - base;
    int nold = 0, off = 0, ap = 0;
    if (v < nv) {
      const int ind = b.valid[(size_t)p * kMaxValid + v];
      nold = slots[ind * 4 + 1 + 2 * kind];
      off = slots[ind * 4 + 2 * kind];
      ap = ao[ind * 2 + kind];
    }
    snold[tid] = nold;
    soff[tid] = off;
    sapp[tid] = ap;
  }
  if (tid == 0) sb[NS] = b.vseg_e[p * NS + NS - 1] - base;
  __syncthreads();
  const int total = sb[NS];
  for (int i = blockIdx.x * 256 + tid; i < total; i += gridDim.x * 256) {
    int lo = 0, hi = NS - 1;  // last segment whose start is <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sb[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int t = i - sb[lo];
    b.vin[base + i] = t < snold[lo] ? pool[soff[lo] + t] : app[sapp[lo] + (t - snold[lo])];
  }
}

// new cube store: valid cubes <- their DS output, every other cube <- old ++ appended.  The
// (kind, cube) sizes go to LDS in coalesced passes; each thread then owns a contiguous run of
// them, so the offsets and the non-empty list need one block scan each.
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_compact_table(MpBuffers b) {
  constexpr int N = 2 * kCubeNum, E = (N + NT - 1) / NT;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* old = slot_table(b, b.pool_cur, p);
  int* nw = slot_table(b, 1 - b.pool_cur, p);
  const int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  __shared__ int16_t vidx[kCubeNum];
  __shared__ int nn[N];
  __shared__ int scratch[NT / 64 + 1];
  for (int s = tid; s < kCubeNum; s += NT) vidx[s] = -1;
  __syncthreads();
  if (tid < nv) vidx[b.valid[(size_t)p * kMaxValid + tid]] = (int16_t)tid;
  __syncthreads();
  int vpts = 0;
  for (int x = tid; x < N; x += NT) {
    const int kind = x / kCubeNum, s = x % kCubeNum, v = vidx[s];
    const int n = v >= 0 ? b.vseg_cnt[p * 2 * kMaxValid + kind * kMaxValid + v] : old[s * 4 + 1 + 2 * kind] + ac[s * 2 + kind];
    nn[x] = n;
    if (v >= 0) vpts += n;
  }
  __syncthreads();
  const int x0 = tid * E, x1 = min(N, x0 + E);
  int sum = 0;
  for (int x = x0; x < x1; ++x) sum += nn[x];
  int run;
  int off = block_excl_scan<NT>(sum, scratch, run);
  for (int x = x0; x < x1; ++x) {  // counts -> offsets, in LDS
    const int c = nn[x];
    nn[x] = off;
    off += c;
  }
  __syncthreads();
  // the table and the non-empty (kind, cube) list written (kind, cube)-consecutive across the lanes
  // (each lane's own run of entries would scatter every store): kind | cube << 1 | (valid + 1) << 14
  // (all passes at once: the non-empty entries ranked by wave ballots, the (pass, wave) counts
  // prefixed by each wave in x order — two barriers instead of three per pass)
  int* items = b.citems + (size_t)p * 2 * kCubeNum;
  constexpr int NW = NT / 64;
  static_assert(NW <= 64, "one count per lane");
  __shared__ int icnt[E][NW];
  const int lane = lane_id(), w = tid >> 6;
  int iex[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int x = e * NT + tid;
    int n = 0;
    if (x < N) {
      const int kind = x / kCubeNum, s = x % kCubeNum, o = nn[x];
      n = (x + 1 < N ? nn[x + 1] : run) - o;
      nw[s * 4 + 2 * kind] = o;
      nw[s * 4 + 1 + 2 * kind] = n;
    }
    const uint64_t m = __ballot(n > 0);
    iex[e] = n > 0 ? __popcll(m & lanemask_lt()) : -1;
    if (lane == 0) icnt[e][w] = __popcll(m);
  }
  __syncthreads();
  int nitems = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int c = lane < NW ? icnt[e][lane] : 0;
    const int incl = wave_incl_scan_x(c);
    const int base = nitems + __shfl(incl - c, w, 64);
    if (iex[e] >= 0) {
      const int x = e * NT + tid;
      items[base + iex[e]] = (x / kCubeNum) | ((x % kCubeNum) << 1) | (((int)vidx[x % kCubeNum] + 1) << 14);
    }
    nitems += __shfl(incl, NW - 1, 64);
  }
  vpts = block_reduce<NT>(vpts, scratch, [](int a, int c) { return a + c; });
  if (tid == 0) {
    b.nitems[p] = nitems;
    b.istate[(size_t)p * kMpStateInts + kMiValidPts] = vpts;
    if (run > b.map_cap) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_MAP;
  }
}

__global__ __launch_bounds__(256) void k_mp_compact_copy(MpBuffers b) {
  const int p = blockIdx.y;
  const int err = b.istate[(size_t)p * kMpStateInts + kMiErr];
  if (err & ERR_CAP_MAP) return;
  const int* old = slot_table(b, b.pool_cur, p);
  const int* nw = slot_table(b, 1 - b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  float4* npool = b.pool + ((size_t)(1 - b.pool_cur) * b.P + p) * b.map_cap;
  const int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  const float4* app = b.app + (size_t)p * b.cap_stack;
  const int* items = b.citems + (size_t)p * 2 * kCubeNum;
  const int nitems = b.nitems[p];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int code = items[it];
    const int kind = code & 1, s = (code >> 1) & 8191, v = (code >> 14) - 1;
    const int n = nw[s * 4 + 1 + 2 * kind];
    const int dst = nw[s * 4 + 2 * kind];
    if (v >= 0) {
      const int b0 = b.vseg_b[p * 2 * kMaxValid + kind * kMaxValid + v];
      for (int t = threadIdx.x; t < n; t += 256) npool[dst + t] = b.vout[b0 + t];
    } else {
      const int nold = old[s * 4 + 1 + 2 * kind], off = old[s * 4 + 2 * kind];
      for (int t = threadIdx.x; t < n; t += 256)
        npool[dst + t] = t < nold ? pool[off + t] : app[ao[s * 2 + kind] + (t - nold)];
    }
  }
}

// k_mp_register workgroups per instance (streaming and lanes; the batch registers nothing)
#ifndef LOAM_REG_WG
#define LOAM_REG_WG 8
#endif
constexpr int kMpRegWg = LOAM_REG_WG;
__global__ __launch_bounds__(256) void k_mp_register(MpBuffers b, MpInput in) {
  const int p = blockIdx.y;
  const loampose::MapRot r = rot_load(b, p);
  const int n = min(in.nfull[p * in.nfull_stride], b.capS);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    b.reg[(size_t)p * b.capS + i] = loampose::point_to_map(r, in.full[(size_t)p * in.full_stride + i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) b.nreg[p] = n;
}

// the hash table size of a FromMap of cap points
int mp_table_size(int cap) {
  const int t = next_pow2(cap) > (1 << 20) ? (1 << 20) : next_pow2(cap);
  return t < 64 ? 64 : t;  // >= 64 buckets: a 3x3x3 search never lists a bucket twice (cell_hash)
}
}  // namespace

// ---------------------------------------------------------------- host side
// A working set's two allocation groups (mp_dev.hpp), the parts of mp_alloc and of mp_loc.hip's
// sets: a buffer of the L-M is listed here and in mp_free, nowhere else.
void mp_alloc_solve(DevAlloc& A, MpBuffers& b, int P, size_t vg_pts, size_t vg_segs) {
  const size_t Ps = (size_t)P * b.cap_stack;
  A(&b.state, (size_t)P * kMpStateFloats * sizeof(float));
  A(&b.istate, (size_t)P * kMpStateInts * sizeof(int));
  A(&b.valid, (size_t)P * kMaxValid * sizeof(int));
  A(&b.vpre, (size_t)P * (kMaxValid + 1) * 2 * sizeof(int));
  A(&b.nfrom, (size_t)P * 2 * sizeof(int));
  A(&b.hC_T, (size_t)P * sizeof(int));
  A(&b.hS_T, (size_t)P * sizeof(int));
  A(&b.stack2, Ps * sizeof(float4));
  A(&b.stack, Ps * sizeof(float4));
  A(&b.sseg_b, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_e, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_cnt, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_leaf, (size_t)P * 2 * sizeof(float));
  // (the stack job's big-segment split: 2P parents, points / outputs like the stacks)
  if (A.err == hipSuccess) A.err = vg_scratch_alloc(b.vg, vg_pts, vg_segs, 2 * P, Ps);
  A(&b.q_ok, Ps * sizeof(int8_t));
  A(&b.q_cf, Ps * sizeof(float4));
  A(&b.q_nn, Ps * 2 * sizeof(int4));
  A(&b.q_fit, Ps * 4 * sizeof(float4));
  A(&b.part, (size_t)P * std::max(kMpSmallGrid, kMpFitGridMax) * 28 * sizeof(double));
  A(&b.rot, (size_t)P * 6 * sizeof(double));
  A(&b.done, (size_t)P * sizeof(int));
  A(&b.ls_epoch, sizeof(unsigned long long));  // (k_mp_lm_begin advances it for one instance)
  if (A.err == hipSuccess) A.err = hipMemset(b.state, 0, (size_t)P * kMpStateFloats * sizeof(float));
  if (A.err == hipSuccess) A.err = hipMemset(b.istate, 0, (size_t)P * kMpStateInts * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(b.done, 0, (size_t)P * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(b.ls_epoch, 0, sizeof(unsigned long long));
}

void mp_alloc_from(DevAlloc& A, MpBuffers& b, int P, int cap) {
  b.map_cap = cap;
  b.tmax = mp_table_size(cap);
  const size_t Pm = (size_t)P * cap;
  A(&b.from, Pm * sizeof(float4));
  A(&b.hC_pts, Pm * sizeof(float4));
  A(&b.hS_pts, Pm * sizeof(float4));
  A(&b.hC_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hS_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hC_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  A(&b.hS_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  // bucket counters: one set per cloud kind (corner, surf: built concurrently)
  A(&b.h_fill, (size_t)2 * P * b.tmax * sizeof(int));
}

hipError_t mp_alloc(MpBuffers& b, int P, int R, int cap_pts, int map_cap, int max_iter, bool batch) {
  DevAlloc A;
  b.P = P;
  b.capC = kLessSharpPerRing * R;
  b.capS = cap_pts;
  b.cap_stack = b.capC + b.capS;
  b.max_iter = max_iter;
  b.pool_cur = 0;
  const size_t Pm = (size_t)P * map_cap, Ps = (size_t)P * b.cap_stack;
  mp_alloc_from(A, b, P, map_cap);
  // the VoxelGrid scratch: sort arrays over the cube inputs or the stacks, a list entry per cube
  // segment.  (The group's zeroes are mp_reset's over again.)
  mp_alloc_solve(A, b, P, std::max(Pm, Ps), (size_t)P * 2 * kMaxValid);
  // the store, the inputs, the insertion and the per-cube VoxelGrid: a mapping set's alone
  A(&b.slots, (size_t)2 * P * kCubeNum * 4 * sizeof(int));
  A(&b.pool, 2 * Pm * sizeof(float4));
  // (a batch set reads the odometry's Last buffers in place and registers no cloud: its inC / inS /
  // inF and reg / nreg stay null)
  if (!batch) {
    A(&b.inC, (size_t)P * b.capC * sizeof(float4));
    A(&b.inS, (size_t)P * b.capS * sizeof(float4));
    A(&b.inF, (size_t)P * b.capS * sizeof(float4));
    A(&b.reg, (size_t)P * b.capS * sizeof(float4));
    A(&b.nreg, (size_t)P * sizeof(int));
  }
  A(&b.in_n, (size_t)P * 3 * sizeof(int));
  A(&b.in_pose, (size_t)P * 6 * sizeof(float));
  A(&b.nstack, (size_t)P * 2 * sizeof(int));
  A(&b.citems, (size_t)P * 2 * kCubeNum * sizeof(int));
  A(&b.nitems, (size_t)P * sizeof(int));
  A(&b.app_cnt, (size_t)P * kCubeNum * 2 * sizeof(int));
  A(&b.app_off, (size_t)P * kCubeNum * 2 * sizeof(int));
  A(&b.app, Ps * sizeof(float4));
  A(&b.vin, Pm * sizeof(float4));
  A(&b.vout, Pm * sizeof(float4));
  int** per_seg[] = {&b.vseg_b, &b.vseg_e, &b.vseg_cnt, &b.vg_lin, &b.vg_mlist, &b.vseg_nold, &b.vseg_skip};
  for (int** q : per_seg) A(q, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_leaf, (size_t)P * 2 * kMaxValid * sizeof(float));
  A(&b.ls_part, (size_t)2 * kMpSmallGrid * 28 * sizeof(double));
  A(&b.ls_flag, (size_t)kMpSmallGrid * sizeof(unsigned long long));
  if (A.err == hipSuccess) A.err = mp_reset(b, nullptr);
  if (A.err == hipSuccess) A.err = hipMemset(b.ls_flag, 0, (size_t)kMpSmallGrid * sizeof(unsigned long long));
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) mp_free(b);
  return A.err;
}

void mp_free(MpBuffers& b) {
  void* ptrs[] = {b.state, b.istate, b.slots, b.pool, b.valid, b.vpre, b.inC, b.inS, b.inF, b.in_n, b.in_pose,
                  b.stack2, b.stack, b.nstack, b.from, b.hC_start, b.hS_start, b.hC_rec, b.hS_rec, b.h_fill, b.hC_T, b.hS_T,
                  b.hC_pts, b.hS_pts, b.nfrom, b.q_ok, b.q_cf, b.q_nn, b.q_fit, b.citems, b.nitems, b.app_cnt, b.app_off, b.app, b.vin, b.vout,
                  b.vseg_b, b.vseg_e, b.vseg_cnt, b.vseg_leaf, b.sseg_b, b.sseg_e, b.sseg_cnt, b.sseg_leaf,
                  b.vg_lin, b.reg, b.nreg, b.part, b.done, b.rot, b.vg_mlist, b.vseg_nold, b.vseg_skip, b.ls_part,
                  b.ls_flag, b.ls_epoch};
  if (b.upd_pending && b.upd_done) (void)hipEventSynchronize(b.upd_done);
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  vg_scratch_free(b.vg);
  if (b.upd_fork) (void)hipEventDestroy(b.upd_fork);
  if (b.upd_done) (void)hipEventDestroy(b.upd_done);
  b = MpBuffers();
}

__global__ void k_mp_reset(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b.P) return;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  ist[kMiCenW] = 10; ist[kMiCenH] = 5; ist[kMiCenD] = 10;  // :64-66
}

hipError_t mp_reset(MpBuffers& b, hipStream_t st, bool both_tables) {
  mp_wait_update(b, st);
  b.pool_cur = 0;
  hipError_t e = hipMemsetAsync(b.state, 0, (size_t)b.P * kMpStateFloats * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(b.done, 0, (size_t)b.P * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(b.istate, 0, (size_t)b.P * kMpStateInts * sizeof(int), st);
  // (pool 0's slot table first: the one the next frame reads)
  if (e == hipSuccess) e = hipMemsetAsync(b.slots, 0, (size_t)(both_tables ? 2 : 1) * b.P * kCubeNum * 4 * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mp_reset, dim3((b.P + 255) / 256), dim3(256), 0, st, b);
  return hipGetLastError();
}

void mp_wait_update(MpBuffers& b, hipStream_t st) {
  if (!b.upd_pending) return;
  b.note(hipStreamWaitEvent(st, b.upd_done, 0));
  b.upd_pending = false;
}

// The stages of a mapping frame that the localization shares (mp_loc.hip; declared in mp_dev.hpp): the
// two core kernels it launches, the stack VoxelGrid, the FromMap hash builds, the L-M loop.
void mp_launch_stack(MpBuffers& b, const MpInput& in, hipStream_t st) {
  hipLaunchKernelGGL(k_mp_stack, dim3(16, b.P), dim3(256), 0, st, b, in);
}
// (reads the final pose and the full cloud only, not the store)
void mp_launch_register(MpBuffers& b, const MpInput& in, hipStream_t st) {
  hipLaunchKernelGGL(k_mp_register, dim3(kMpRegWg, b.P), dim3(256), 0, st, b, in);
}

void mp_stack_vg(MpBuffers& b, int P, hipStream_t vs, int stack_max) {
  VgJob js = b.vg.job();
  js.in = b.stack2; js.out = b.stack; js.begin = b.sseg_b; js.end = b.sseg_e; js.leaf = b.sseg_leaf;
  js.out_count = b.sseg_cnt; js.nseg = 2 * P; js.total = P * b.cap_stack;
  // two large segments per instance (the fused 12288-point kernel); when the host knows both fit
  // (streaming), the cascade's finish is not enqueued
  js.zeroed = true;
  b.note(vg_route_stack(js, vs, P, stack_max, b.tune.vg_split, b.capS, &b.vg.split));
}

void mp_hash_from(MpBuffers& b, int P, hipStream_t st, bool spread) {
  HashJob hc;
  hc.pts = b.from; hc.pts_stride = b.map_cap; hc.pts_off = nullptr; hc.pts_off_stride = 0;
  hc.count = b.nfrom; hc.count_stride_bytes = 2 * sizeof(int);
  hc.start = b.hC_start; hc.fill = b.h_fill; hc.out = b.hC_pts; hc.tsize = b.hC_T; hc.tmax = b.tmax;
  hc.inv_h = 1.0f;
  hc.shift = 0;  // the 5-NN search scans whole buckets: keep them to single cells
  hc.chunks = nullptr;
  hc.rec = b.hC_rec;
  HashJob hs = hc;
  hs.rec = b.hS_rec;
  hs.pts_off = b.nfrom; hs.pts_off_stride = 2;
  hs.count = b.nfrom + 1; hs.start = b.hS_start; hs.out = b.hS_pts; hs.tsize = b.hS_T;
  hs.fill = b.h_fill + (size_t)P * b.tmax;  // (the two indexes are built in one launch / concurrently)
  hash_build_pair(hc, hs, P, st, false, spread ? HashForm::kGrid : HashForm::kAuto);
}

void mp_lm_loop(MpBuffers& b, int P, hipStream_t st, Prof* prof, bool map_empty, bool persist) {
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  hipLaunchKernelGGL(k_mp_lm_begin, dim3((P + 255) / 256), dim3(256), 0, st, b);
  // workgroups per instance: all the stack's queries at once for a few instances; for large
  // batches about one pass over a VLP-16 stack (bigger stacks loop), fewer idle workgroups
  const int gq = std::min(P >= 64 ? 24 : 64, (b.cap_stack + kMpQueryThreads - 1) / kMpQueryThreads);
  // an empty map store (the first frame after a reset) cannot run the L-M (:706): no launches
  // one instance (streaming): the whole L-M loop as one persistent launch (tuning mp_persist)
  const int gls = persist && P == 1 && !map_empty && b.tune.mp_persist ? mp_lm_stream_grid() : 0;
  if (gls > 0) {
    hipLaunchKernelGGL(k_mp_lm_stream, dim3(gls), dim3(kMpQueryThreads), 0, st, b);
    mark("k_mp_lm_stream");
  }
  for (int it = 0; it < (map_empty || gls > 0 ? 0 : b.max_iter); ++it) {
    if (P <= b.tune.mp_small_max) {  // small batches: one launch per iteration
      hipLaunchKernelGGL(k_mp_lm_small, dim3(kMpSmallGrid, P), dim3(kMpQueryThreads), 0, st, b);
      mark("k_mp_lm_small");
      continue;
    }
    // (P >= 512: 64 workgroups, two passes per lane over a VLP-16 stack; round 6 at 1024 problems:
    // 12.28-12.32 -> 12.20-12.23 ms/step against 96; at 128 the one-pass 96 stays best)
    const int gfit_auto = P >= 512 ? 64 : gq * (kMpQueryThreads / kMpFitThreads);
    const int gfit = std::min(kMpFitGridMax, b.tune.fit_wg > 0 ? b.tune.fit_wg : gfit_auto);
    // search + fit (+ step) in one launch (round 3's separate k_mp_nn / k_mp_fit launches, and 2 / 4
    // lanes per query, measured slower and were removed in round 6)
    const bool fused = P <= b.tune.mp_fused_max;
    if (fused && prof) hipLaunchKernelGGL((k_mp_nnfit<true, true>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else if (fused) hipLaunchKernelGGL((k_mp_nnfit<true, false>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else if (prof) hipLaunchKernelGGL((k_mp_nnfit<false, true>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else hipLaunchKernelGGL((k_mp_nnfit<false, false>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    mark("k_mp_nnfit");
    if (!fused) {
      hipLaunchKernelGGL(k_mp_iter<kMpThreads>, dim3(P), dim3(kMpThreads), 0, st, b);
      mark("k_mp_iter");
    }
  }
  hipLaunchKernelGGL(k_mp_lm_end, dim3((P + 255) / 256), dim3(256), 0, st, b);
}

// ---- the stages of a mapping frame; every caller composes the ones whose results it hands out ----
namespace {
// front: the pose and the valid cubes, the stacks and their VoxelGrid, FromMap and its hashes.
// from_map = false: the store was just reset (batch frame 1), FromMap is empty by construction and
// neither gathered nor hashed (k_mp_prepare has set nfrom and the valid count to 0; no L-M runs)
void mp_front(MpBuffers& b, const MpInput& in, hipStream_t st, Prof* prof, int stack_max, const SideStream* side,
              bool from_map) {
  const int P = b.P;
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  mp_wait_update(b, st);  // (the previous frame's map update, when it was deferred)
  hipLaunchKernelGGL(k_mp_prepare, dim3(P), dim3(kMpThreads), 0, st, b, in);
  mark("k_mp_prepare");
  mp_launch_stack(b, in, st);
  mark("k_mp_stack");
  if (side && side->inputs_read) b.note(hipEventRecord(side->inputs_read, st));  // (in.corner / in.surf read)
  // the stack VoxelGrid: with a side stream it runs there, beside the FromMap gather and the map
  // hash builds (which read only the store)
  const bool fork = side && side->st && !prof && from_map;
  if (fork) {
    b.note(hipEventRecord(side->fork, st));
    b.note(hipStreamWaitEvent(side->st, side->fork, 0));
  }
  mp_stack_vg(b, P, fork ? side->st : st, stack_max);
  if (fork) b.note(hipEventRecord(side->join, side->st));
  mark("vg_stack");
  if (!from_map) return;
  hipLaunchKernelGGL(k_mp_gather, dim3(32, P), dim3(256), 0, st, b);
  mark("k_mp_gather");
  mp_hash_from(b, P, st);
  mark("k_hash_build_map");
  if (fork) b.note(hipStreamWaitEvent(st, side->join, 0));
}

// the map update on us: insertion + per-valid-cube downsampling into the other pool, which becomes
// the current one (k_mp_lm_end zeroed the cascade's list counters)
void mp_update(MpBuffers& b, hipStream_t us, Prof* prof) {
  const int P = b.P;
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  // a few instances: 1024 threads per instance (the per-instance serial parts are the cost)
  // 1024 threads per instance also for batches (k_mp_insert 0.40 -> 0.25 ms/step at batch 1024 against 256)
  hipLaunchKernelGGL(k_mp_insert<1024>, dim3(P), dim3(1024), 0, us, b, (int*)b.vg.keys, (int*)b.vg.vals);
  mark("k_mp_insert");
  hipLaunchKernelGGL(k_mp_vseg, dim3(P), dim3(kMpThreads), 0, us, b);
  hipLaunchKernelGGL(k_mp_vcopy, dim3(32, P), dim3(256), 0, us, b);
  mark("k_mp_vseg_vcopy");
  VgJob jv = b.vg.job();
  jv.in = b.vin; jv.out = b.vout; jv.begin = b.vseg_b; jv.end = b.vseg_e; jv.leaf = b.vseg_leaf;
  jv.out_count = b.vseg_cnt; jv.nseg = 2 * kMaxValid * P; jv.total = P * b.map_cap;
  // only the non-empty segments, listed by k_mp_vseg (k_mp_lm_end zeroed the counters)
  jv.list = b.vg_lin; jv.list_n = b.vg.counts + 2; jv.zeroed = true;
  b.note(vg_route_cubes(jv, us, P, b.tune.vg_merge, b.vseg_nold, b.vg_mlist, b.vg.counts + 3, b.vseg_skip));
  mark("vg_cubes");
  hipLaunchKernelGGL(k_mp_compact_table<1024>, dim3(P), dim3(1024), 0, us, b);
  hipLaunchKernelGGL(k_mp_compact_copy, dim3(64, P), dim3(256), 0, us, b);
  mark("k_mp_compact");
  b.pool_cur = 1 - b.pool_cur;
}

// an instance's frame counters (its istate row q) added to the statistics
void mp_stats_add(loam_stats& s, const int* q) {
  s.mp_iters += q[kMiIters];
  s.mp_rows_sum += (uint64_t)q[kMiRows];
  s.mp_stack += (uint64_t)(q[kMiStackC] + q[kMiStackS]);
  s.mp_stack_iters += (uint64_t)q[kMiIters] * (q[kMiStackC] + q[kMiStackS]);
  s.mp_fits += (uint64_t)q[kMiFits];
  s.mp_map_points += (uint64_t)(q[kMiFromC] + q[kMiFromS]);
  s.mp_map_valid_points += (uint64_t)q[kMiValidPts];
  s.mp_degenerate_steps += (uint64_t)q[kMiDegSteps];
  s.mp_grid_shifts += (uint64_t)q[kMiShifts];
  s.mp_nn_candidates += (uint64_t)(uint32_t)q[kMiNnCand];
  s.mp_nn_cells += (uint64_t)(uint32_t)q[kMiNnCells];
}
}  // namespace

void mp_frame(MpBuffers& b, const MpInput& in, hipStream_t st, Prof* prof,
              const std::function<void()>& before_register, int stack_max, hipStream_t defer) {
  mp_front(b, in, st, prof, stack_max, nullptr, /*from_map=*/true);
  mp_lm_loop(b, b.P, st, prof, false, /*persist=*/true);
  // defer: the map update on the other stream, forked here; the registration stays on st
  if (defer) {
    if (!b.upd_fork) b.note(hipEventCreateWithFlags(&b.upd_fork, hipEventDisableTiming));
    if (!b.upd_done) b.note(hipEventCreateWithFlags(&b.upd_done, hipEventDisableTiming));
    b.note(hipEventRecord(b.upd_fork, st));
    b.note(hipStreamWaitEvent(defer, b.upd_fork, 0));
  }
  mp_update(b, defer ? defer : st, prof);
  if (defer) {
    b.note(hipEventRecord(b.upd_done, defer));
    b.upd_pending = true;
  }
  if (before_register) before_register();
  mp_launch_register(b, in, st);
  if (prof) prof->mark("k_mp_register");
}

// the frame's kernels on `in` and the downloads (both stream entry points); hook: called just
// before k_mp_register (the late full-cloud staging); defer: the map update's stream (mp_frame),
// nullptr = in order on st
template <typename Hook>
int mp_stream_run(MpBuffers& b, hipStream_t st, const MpInput& in, const int* n, loam_pose6* aft, loam_pose6* bef,
                  loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                  bool* updated, Hook hook, hipStream_t defer) {
  const hipEvent_t e0 = io.e0, e1 = io.e1;
  hipError_t le = hipEventRecord(e0, st);
  mp_frame(b, in, st, nullptr, [&]() {
    if (le != hipSuccess) return;
    le = hook();
  }, std::max(n[0], n[1]), defer);
  if (le == hipSuccess) le = hipEventRecord(e1, st);
  // a deferred update's valid-point count (stats) into the mapped host block after it, one slot
  // per frame parity: this call reads the previous frame's (complete: this frame's kernels on st
  // waited for that update), while this frame's may still be writing the other slot
  const bool deferred = defer && b.upd_pending;
  if (deferred && le == hipSuccess) {
    Xfer xg;
    xg.get(io.xb.d + kXferMpUpd + 4 * (1 - b.pool_cur), b.istate + kMiValidPts, sizeof(int));
    le = xfer_launch(xg, defer);
    if (le == hipSuccess) le = hipEventRecord(b.upd_done, defer);
  }
  // state (kMpStateFloats), istate (kMpStateInts), nreg into the mapped host block, one launch
  static_assert(kXferMp + 4 * (kMpStateFloats + kMpStateInts + 1) <= kXferMpUpd, "mapping transfer region");
  static_assert(kXferMpUpd + 8 <= kXferBytes, "deferred valid-point slots");
  const float* sf = (const float*)(io.xb.h + kXferMp);
  const int* si = (const int*)(io.xb.h + kXferMp) + kMpStateFloats;
  const int* pnreg = si + kMpStateInts;
  {
    Xfer xg;
    char* d = io.xb.d + kXferMp;
    xg.get(d, b.state, kMpStateFloats * sizeof(float));
    xg.get(d + kMpStateFloats * 4, b.istate, kMpStateInts * sizeof(int));
    xg.get(d + (kMpStateFloats + kMpStateInts) * 4, b.nreg, sizeof(int));
    le = le == hipSuccess ? xfer_launch(xg, st) : le;
  }
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  const int nreg = *pnreg;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (he == hipSuccess) he = b.take_error();
  if (he == hipSuccess) he = le;
  if (he != hipSuccess) {
    err = std::string("mapping: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  if (si[kMiErr]) {
    err = "mapping capacity exceeded (map store / stack)";
    return LOAM_E_CAPACITY;
  }
  std::memcpy(aft, sf + kMpAft, sizeof(loam_pose6));
  std::memcpy(bef, sf + kMpBef, sizeof(loam_pose6));
  if (updated) *updated = si[kMiLmRan] != 0;
  int rc = LOAM_OK;
  if (registered) {
    if ((uint32_t)nreg > registered->capacity) {
      registered->count = (uint32_t)nreg;
      err = "registered cloud capacity too small";
      rc = LOAM_E_CAPACITY;
    } else {
      registered->count = (uint32_t)nreg;
      pin.reset();
      he = pin.down(st, registered->pts, b.reg, (size_t)nreg);
      if (he == hipSuccess) he = hipStreamSynchronize(st);
      if (he != hipSuccess) {
        err = std::string("registered cloud download: ") + hipGetErrorString(he);
        return LOAM_E_HIP;
      }
      pin.finish();
    }
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    mp_stats_add(*stats, si);
    // (a deferred update: the previous frame's map, this frame's is not counted yet)
    if (deferred) stats->mp_map_valid_points = (uint64_t)*(const int*)(io.xb.h + kXferMpUpd + 4 * b.pool_cur);
    stats->ms_mp = ms;
  }
  return rc;
}

int mp_stream_frame(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const loam_cloud_out& corner,
                    const loam_cloud_out& surf, const loam_cloud_out& full, loam_pose6* aft, loam_pose6* bef,
                    loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                    const float* imu_rp, bool* updated, hipStream_t st2, hipEvent_t ev2, hipStream_t defer) {
  if (corner.count > (uint32_t)b.capC || surf.count > (uint32_t)b.capS || full.count > (uint32_t)b.capS) {
    err = "mapping input cloud exceeds capacity";
    return LOAM_E_CAPACITY;
  }
  if ((corner.count && !corner.pts) || (surf.count && !surf.pts) || (full.count && !full.pts)) {
    err = "mapping input cloud pts is null";
    return LOAM_E_INVAL;
  }
  // host inputs: [0..2] counts, [4..9] pose, [10..11] IMU (roll, pitch), [12] IMU flag, to the
  // device in one k_xfer launch; downloads through io.xb (mp_stream_run)
  int mi[16];
  int* n = mi;
  n[0] = (int)corner.count; n[1] = (int)surf.count; n[2] = (int)full.count;
  std::memcpy(mi + 4, &odom_sum, 6 * sizeof(float));
  const float rp[2] = {imu_rp ? imu_rp[0] : 0.0f, imu_rp ? imu_rp[1] : 0.0f};
  std::memcpy(mi + 10, rp, sizeof(rp));
  mi[12] = imu_rp ? 1 : 0;
  pin.reset();
  // room for all three clouds now: the full cloud is staged later, while the kernels run
  hipError_t ue = pin.reserve((size_t)n[0] + n[1] + n[2], st);
  if (ue == hipSuccess) ue = pin.up(st, b.inC, corner.pts, (size_t)n[0]);
  if (ue == hipSuccess) ue = pin.up(st, b.inS, surf.pts, (size_t)n[1]);
  // only k_mp_register reads the full cloud: with a second stream its staging copy and DMA
  // overlap the frame's kernels (enqueued just before k_mp_register)
  const bool late = st2 != nullptr && n[2] > 0;
  if (ue == hipSuccess && !late) ue = pin.up(st, b.inF, full.pts, (size_t)n[2]);
  if (ue == hipSuccess) {
    Xfer xp;
    xp.put(b.in_n, n, 3 * sizeof(int));
    xp.put(b.in_pose, mi + 4, 6 * sizeof(float));
    xp.put(b.state + kMpImuRP, mi + 10, 2 * sizeof(float));
    xp.put(b.istate + kMiImu, mi + 12, sizeof(int));
    ue = xfer_launch(xp, st);
  }
  if (ue != hipSuccess) {
    err = std::string("mapping upload: ") + hipGetErrorString(ue);
    return LOAM_E_HIP;
  }
  MpInput in;
  in.corner = b.inC; in.surf = b.inS; in.full = b.inF;
  in.corner_stride = b.capC; in.surf_stride = b.capS; in.full_stride = b.capS;
  in.ncorner = b.in_n; in.nsurf = b.in_n + 1; in.nfull = b.in_n + 2;
  in.ncorner_stride = in.nsurf_stride = in.nfull_stride = 3;
  in.pose = b.in_pose; in.pose_stride = 6;
  return mp_stream_run(b, st, in, n, aft, bef, registered, stats, err, pin, io, updated, [&]() {
    if (!late) return hipSuccess;
    hipError_t le = pin.up(st2, b.inF, full.pts, (size_t)n[2]);
    if (le == hipSuccess) le = hipEventRecord(ev2, st2);
    if (le == hipSuccess) le = hipStreamWaitEvent(st, ev2, 0);
    return le;
  }, defer);
}

// the device-resident chain (loam_chain_sweep): the clouds are already on the device (odometry's
// published Last / full-end buffers, src, with device counts); n3: their counts on the host
int mp_stream_frame_dev(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const MpInput& src, const int* n3,
                        loam_pose6* aft, loam_pose6* bef, loam_cloud_out* registered, loam_stats* stats,
                        std::string& err, Staging& pin, const StreamIo& io, const float* imu_rp, bool* updated,
                        hipStream_t defer) {
  if (n3[0] > b.capC || n3[1] > b.capS || n3[2] > b.capS) {
    err = "mapping input cloud exceeds capacity";
    return LOAM_E_CAPACITY;
  }
  // as mp_stream_frame: the pose, the IMU (roll, pitch) and flag in one k_xfer launch
  const float rp[2] = {imu_rp ? imu_rp[0] : 0.0f, imu_rp ? imu_rp[1] : 0.0f};
  const int flag = imu_rp ? 1 : 0;
  Xfer xp;
  xp.put(b.in_pose, &odom_sum, 6 * sizeof(float));
  xp.put(b.state + kMpImuRP, rp, sizeof(rp));
  xp.put(b.istate + kMiImu, &flag, sizeof(int));
  const hipError_t ue = xfer_launch(xp, st);
  if (ue != hipSuccess) {
    err = std::string("mapping upload: ") + hipGetErrorString(ue);
    return LOAM_E_HIP;
  }
  MpInput in = src;
  in.pose = b.in_pose;
  in.pose_stride = 6;
  return mp_stream_run(b, st, in, n3, aft, bef, registered, stats, err, pin, io, updated,
                       []() { return hipSuccess; }, defer);
}

// /laser_cloud_surround input (:1042-1047): every in-bounds cube of the 5x5x5 neighbourhood of the
// frame's centre cube (laserCloudSurroundInd, :617-670, FOV test or not) in (i, j, k) loop order,
// each cube's corner points then its surf points, from the store the frame left; one VoxelGrid
// segment (leaf 0.2, downSizeFilterCorner) over vin.
__global__ __launch_bounds__(256) void k_mp_surround(MpBuffers b) {
  const int tid = threadIdx.x;
  if (tid == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; }  // (its VoxelGrid's lists)
  const int* ist = b.istate;
  const int* slots = slot_table(b, b.pool_cur, 0);
  const float4* pool = b.pool + (size_t)b.pool_cur * b.P * b.map_cap;
  __shared__ int sh_ind[kMaxValid], sh_pre[kMaxValid + 1], sh_n;
  if (tid == 0) {
    const int cI = ist[kMiCubeI], cJ = ist[kMiCubeJ], cK = ist[kMiCubeK];
    int n = 0, acc = 0;
    for (int i = cI - 2; i <= cI + 2; ++i)
      for (int j = cJ - 2; j <= cJ + 2; ++j)
        for (int k = cK - 2; k <= cK + 2; ++k) {
          if (!(i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD)) continue;
          const int ind = cube_index(i, j, k);
          sh_ind[n] = ind;
          sh_pre[n] = acc;
          acc += slots[ind * 4 + 1] + slots[ind * 4 + 3];
          ++n;
        }
    sh_pre[n] = acc;
    sh_n = n;
    b.vseg_b[0] = 0;
    b.vseg_e[0] = acc;
    b.vseg_leaf[0] = 0.2f;
  }
  __syncthreads();
  const int n = sh_n;
  for (int c = 0; c < n; ++c) {
    const int ind = sh_ind[c], nc = slots[ind * 4 + 1], ns = slots[ind * 4 + 3];
    const int oc = slots[ind * 4 + 0], os = slots[ind * 4 + 2];
    float4* dst = b.vin + sh_pre[c];
    for (int t = tid; t < nc + ns; t += 256) dst[t] = t < nc ? pool[oc + t] : pool[os + (t - nc)];
  }
}

int mp_stream_surround(MpBuffers& b, hipStream_t st, loam_cloud_out* out, std::string& err) {
  mp_wait_update(b, st);  // (the last frame's map update, when deferred)
  hipLaunchKernelGGL(k_mp_surround, dim3(1), dim3(256), 0, st, b);
  VgJob j = b.vg.job();
  j.in = b.vin; j.out = b.vout; j.begin = b.vseg_b; j.end = b.vseg_e; j.leaf = b.vseg_leaf;
  j.out_count = b.vseg_cnt; j.nseg = 1; j.total = b.P * b.map_cap;
  j.zeroed = true;  // (by k_mp_surround)
  b.note(vg_route_surround(j, st));
  int cnt = 0;
  hipError_t he = hipMemcpyAsync(&cnt, b.vseg_cnt, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = b.take_error();
  if (he != hipSuccess) {
    err = std::string("surround: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  if ((uint32_t)cnt > out->capacity) {
    out->count = (uint32_t)cnt;
    err = "surround cloud capacity too small";
    return LOAM_E_CAPACITY;
  }
  out->count = (uint32_t)cnt;
  if (cnt && hipMemcpy(out->pts, b.vout, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) {
    err = "surround download failed";
    return LOAM_E_HIP;
  }
  return LOAM_OK;
}

// A batch problem ends at cur's solved pose: no call returns its map or its registered clouds, so
// the batch frames build neither the registered clouds nor the map with cur inserted.
namespace {
// the corner / surf clouds of the odometry's Last[buf] (the batch frames read no full cloud)
MpInput batch_input(const OdBuffers& od, int buf) {
  MpInput in;
  in.corner = od.lastC + (size_t)buf * od.P * od.capC;
  in.surf = od.lastS + (size_t)buf * od.P * od.capS;
  in.full = nullptr;
  in.corner_stride = od.capC; in.surf_stride = od.capS; in.full_stride = 0;
  in.ncorner = od.nlast + buf * 2; in.nsurf = od.nlast + buf * 2 + 1; in.nfull = nullptr;
  in.ncorner_stride = 2 * kOdBufs; in.nsurf_stride = 2 * kOdBufs; in.nfull_stride = 0;
  return in;
}
}  // namespace

// frame 1 of the batch problem: reset, then prev (the seed's Last[buf]) into the empty store at
// the zero pose.  Reads only what the odometry seeding wrote, so it may run beside od_solve.
// The store is empty by construction: no FromMap gather or hash build, no L-M launches
// (k_mp_lm_begin / k_mp_lm_end still set the state frame 2 reads and zero the cascade's counters),
// then the map update, which leaves prev's map in pool 1 for frame 2.
void mp_batch_frame1(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof, const SideStream* side) {
  // (only pool 0's slot table, which this frame reads, must be empty: k_mp_compact_table writes
  // every entry of pool 1's)
  b.note(mp_reset(b, st, /*both_tables=*/false));
  if (prof) prof->mark("mp_reset");
  MpInput in = batch_input(od, buf);
  in.pose = nullptr; in.pose_stride = 0;
  mp_front(b, in, st, prof, -1, side, /*from_map=*/false);
  mp_lm_loop(b, b.P, st, prof, /*map_empty=*/true, /*persist=*/true);
  mp_update(b, st, prof);
}

// frame 2: cur (TransformToEnd's Last[buf]) with the odometry transformSum, up to its solved pose
// (k_mp_lm_end); the store stays prev's map (pool 1) until the next step's reset
void mp_batch_frame2(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof, const SideStream* side) {
  MpInput in = batch_input(od, buf);
  in.pose = od.state + kOdSum; in.pose_stride = kOdStateFloats;
  mp_front(b, in, st, prof, -1, side, /*from_map=*/true);
  mp_lm_loop(b, b.P, st, prof, false, /*persist=*/true);
  if (prof) prof->mark("k_mp_lm_end");  // (no later mark of the step would take it)
}

// per-instance mapping L-M iteration counts of the last frame (loam_batch_iterations)
hipError_t mp_batch_iters(MpBuffers& b, hipStream_t st, int32_t* iters) {
  std::vector<int> si((size_t)b.P * kMpStateInts);
  hipError_t he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = hipMemcpy(si.data(), b.istate, si.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (he == hipSuccess)
    for (int p = 0; p < b.P; ++p) iters[p] = si[(size_t)p * kMpStateInts + kMiIters];
  return he;
}

int mp_batch_download(MpBuffers& b, hipStream_t st, loam_pose6* aft, loam_stats* stats, std::string& err) {
  std::vector<float> sf((size_t)b.P * kMpStateFloats);
  std::vector<int> si((size_t)b.P * kMpStateInts);
  hipError_t he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = b.take_error();
  if (he == hipSuccess) he = hipMemcpy(sf.data(), b.state, sf.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(si.data(), b.istate, si.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (he != hipSuccess) {
    err = std::string("mapping: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  for (int p = 0; p < b.P; ++p) {
    const int* q = &si[(size_t)p * kMpStateInts];
    if (q[kMiErr]) {
      err = "mapping capacity exceeded (map store / stack)";
      return LOAM_E_CAPACITY;
    }
    if (aft) std::memcpy(&aft[p], &sf[(size_t)p * kMpStateFloats + kMpAft], sizeof(loam_pose6));
    if (stats) mp_stats_add(*stats, q);
  }
  return LOAM_OK;
}

}  // namespace loam

#ifdef LOAM_PHASES
// the phase sums of the last-workgroup kernel of this file (PhaseAcc, dev_common.hpp); diagnostic
// build only (tools/phase_stream.py)
extern "C" int loam_debug_phases_mp(unsigned long long* out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(loam::g_ph_mp), sizeof(PhaseAcc)) == hipSuccess ? 0 : -1;
}
#endif
