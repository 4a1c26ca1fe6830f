"""Where a k_sr_ring_fused and a k_sr_ringvg workgroup's time goes: mean microseconds per
barrier-delimited phase, from the stamps of the diagnostic build (sr.hip LOAM_SR_PHASES):

    tools/build_variant.sh srph -DLOAM_SR_PHASES
    LOAM_HIP_LIB=loam_velodyne-1_amd/exp/srph.so python tools/sr_phases.py [problems] [steps]

The batch is 64 distinct problems repeated (the ring sort's work does not depend on the scene)."""
import ctypes
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
loam = importlib.import_module("loam_velodyne-1_amd")
sg = importlib.import_module("loam_velodyne-1_amd.synthgen")

NAMES = ("ticket", "loads + sweep ends", "ring ID + orientation", "publish + ranks", "prefix + wait for tiles",
         "ring bases", "scatter")
VG_NAMES = ("candidate copy + gather + bbox", "voxel keys + run heads + lengths", "sort", "voxel heads", "member means")


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lib = loam.lib()
    if not hasattr(lib, "loam_debug_phases_sr"):
        sys.exit("not a -DLOAM_SR_PHASES build (set LOAM_HIP_LIB)")
    p, c = sg.batch_problems(min(P, 64), base_seed=1000)
    prevs, curs = [p[i % len(p)] for i in range(P)], [c[i % len(c)] for i in range(P)]
    e = loam.Engine()
    e.batch_upload(prevs, curs)
    out = (ctypes.c_ulonglong * 8)()
    e.batch_run()
    e.sync()
    assert lib.loam_debug_phases_sr(out) == 0       # (warm-up step dropped)
    vg = (ctypes.c_ulonglong * 8)()
    assert lib.loam_debug_phases_ringvg(vg) == 0
    for _ in range(steps):
        e.batch_run()
    e.sync()
    assert lib.loam_debug_phases_sr(out) == 0
    assert lib.loam_debug_phases_ringvg(vg) == 0
    e.close()
    n = max(int(out[0]), 1)
    tot = sum(int(out[k]) for k in range(1, 8))
    print(f"k_sr_ring_fused, {P} problems, {steps} steps: {int(out[0])} scattering workgroups, "
          f"{tot / n / 100:.2f} us per workgroup")
    for k in range(1, 8):
        print(f"  {NAMES[k - 1]:28s} {int(out[k]) / n / 100:7.2f} us  {100.0 * int(out[k]) / max(tot, 1):5.1f} %")

    n = max(int(vg[0]), 1)
    tot = sum(int(vg[k]) for k in range(1, 6))
    print(f"k_sr_ringvg, {P} problems, {steps} steps: {int(vg[0])} downsampling workgroups, "
          f"{tot / n / 100:.2f} us per workgroup, {int(vg[7]) / n:.0f} runs per ring, "
          f"{100.0 * int(vg[6]) / n:.1f} % of the rings sorted on 32-bit keys")
    for k in range(1, 6):
        print(f"  {VG_NAMES[k - 1]:34s} {int(vg[k]) / n / 100:7.2f} us  {100.0 * int(vg[k]) / max(tot, 1):5.1f} %")


if __name__ == "__main__":
    main()
