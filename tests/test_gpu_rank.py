"""The ring sort's stable rank by bit ballots (dev_common.hpp wave_key_rank): the stand-alone check
against a serial reference (tools/mb/rank_check.hip, built by loam_velodyne-1_amd/Makefile: waves
of one ring, two rings, all R rings for R = 16 and 64, invalid lanes interleaved, no valid lane),
and through the product: a batch of 64 sweeps of 1, 63, 64, 65, 2047, 2048, 2049 and 4097 points
with a NaN at every 97th point, whose ring-sorted full clouds must equal the oracle's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 63, 64, 65, 2047, 2048, 2049, 4097)


def test_rank_helper_against_serial_reference():
    exe = os.path.join(ROOT, "tools", "mb", "rank_check")
    assert os.path.exists(exe), "build first (make -C loam_velodyne-1_amd)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def test_short_sweeps_full_cloud(loam, oc, sg):
    prevs, curs = sg.batch_problems(4, base_seed=4200)
    sweeps = []
    for j in range(64):                       # sweep j: a window of a source sweep, its length from LENGTHS
        src = (prevs + curs)[j % 8]
        n = LENGTHS[(j // 8) % len(LENGTHS)]
        start = 1000 * (j % 8)
        raw = src[start:start + n].copy()
        raw[96::97, 0] = np.nan               # every 97th point (the one-point sweep keeps its point)
        sweeps.append(raw)
    e = loam.Engine()
    e.batch_upload(sweeps[0::2], sweeps[1::2])
    e.batch_run()
    pts, off = e.batch_features(clouds=("full",))["full"]
    e.close()
    worst, exact = 0.0, True
    for j, raw in enumerate(sweeps):
        o = oc.Oracle(oc.default_config(system_delay=1), cap=40000)
        assert o.scan_registration(raw)[0] != 0
        rc, f = o.scan_registration(raw)
        assert rc == 0
        got, want = pts[int(off[j]):int(off[j + 1])], f["full"]
        assert got.shape == want.shape, (j, len(raw), got.shape, want.shape)
        np.testing.assert_array_equal(got[:, :3], want[:, :3], err_msg=f"sweep {j} ({len(raw)} points)")
        worst = max(worst, float(np.max(np.abs(got[:, 3] - want[:, 3]), initial=0.0)))
        exact &= np.array_equal(got.view(np.uint32), want.view(np.uint32))
    print(f"full clouds: largest intensity difference {worst:.3g}")
    assert exact
