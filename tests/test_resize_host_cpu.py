"""CPU: the host half of the frame resize (nr-slam_amd/csrc/nrs_resize_host.hpp: the refusals, the box test, the tap tables at both
borders, the pixel bodies the kernel runs) in a program of its own under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nr-slam_amd")


def test_resize_check_runs_clean():
    p = subprocess.run(["make", "-C", PKG, "resize_check"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "resize_check OK" in p.stdout, p.stdout + p.stderr
    r = subprocess.run([os.path.join(PKG, "resize_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "resize_check OK" and not r.stderr, r.stdout + r.stderr
