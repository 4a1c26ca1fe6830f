"""loam_map_score's per-point search (loam_velodyne-1_amd/csrc/score.hpp score_nearest) visits the
own cell, then those of the other 26 cells whose box is closer than the best so far, through a hash
table whose buckets may hold several cells.  tests/score_check.cpp compiles it for the host, builds
the bucket table as the device build defines it and compares every query's term
(d2 < r2 ? d2 : r2) with a brute-force loop over the whole cloud, bit for bit: seeded random clouds,
queries on cell faces / edges / corners, negative coordinates, a query exactly max_dist from its
only neighbour (not an inlier: the test is strict), an empty table, queries that have no neighbour
by definition, and table sizes 64 and 2^20."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_search_equals_brute_force(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "score_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "score_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    print(r.stderr)
    checked, mismatches = map(int, r.stdout.split())
    assert checked == 76222 and mismatches == 0
    # the cases are no empty ones: inliers and non-inliers at every radius of the random clouds
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("random: 20000 points")]
    assert len(lines) == 3
    for ln in lines:
        inl = int(ln.split(" inliers")[0].split()[-1])
        assert 100 < inl < 2900, ln


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_equals_plain_loop(dtype):
    """tests/score_ref.py (the GPU tests' reference) windows its brute force; here it meets the plain
    loop over the whole cloud: equal bit for bit wherever the plain minimum is below WINDOW^2, and
    nowhere smaller than WINDOW^2 elsewhere"""
    rng = np.random.default_rng(20261103)
    cloud = np.concatenate([rng.normal(0.0, 3.0, (3000, 3)), rng.uniform(-40.0, 40.0, (3000, 3))]).astype(np.float32)
    q = np.concatenate([rng.normal(0.0, 3.0, (400, 3)), rng.uniform(-42.0, 42.0, (400, 3))]).astype(np.float32).astype(dtype)
    got = sr.nearest_d2(sr.SortedMap(cloud), q, dtype)
    m = cloud.astype(dtype)
    dx, dy, dz = (m[None, :, k] - q[:, None, k] for k in range(3))
    plain = (dx * dx + dy * dy + dz * dz).min(axis=1)
    assert plain.dtype == dtype and got.dtype == dtype
    near = plain < dtype(sr.WINDOW) ** 2
    assert 200 < near.sum() < 700
    np.testing.assert_array_equal(got[near], plain[near])
    assert np.all(got[~near] >= dtype(sr.WINDOW) ** 2)
    assert sr.nearest_d2(sr.SortedMap(cloud[:0]), q, dtype).min() == np.inf
