"""CPU: the host half of the stereo rectification (nr-slam_amd/csrc/nrs_rect_host.hpp: the refusals, P R and its inverse, the map of a
pixel, the fixed-point tap rule, the blend -- the bodies the kernels run) in a program of its own under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nr-slam_amd")


def test_rect_check_runs_clean():
    p = subprocess.run(["make", "-C", PKG, "rect_check"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "rect_check OK" in p.stdout, p.stdout + p.stderr
    r = subprocess.run([os.path.join(PKG, "rect_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "rect_check OK" and not r.stderr, r.stdout + r.stderr
