"""CPU: the host side of the image front end (include/nrs.h f5) -- the new entry points are declared, listed and exported; the Masker
mirror of nr-slam_amd/host/nrs_views.hpp compiles with plain g++ and parses the reference's filters.txt files (tests/golden/filters)."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_front_configure", "nrs_front_process", "nrs_klt_set_reference_front", "nrs_klt_track_front", "nrs_shi_extract_front"]

MAIN = r"""
#include <cstdio>
#include <fstream>
#include "nrs_views.hpp"
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::ifstream in(argv[a]);
        if (!in.is_open()) return 2;
        for (const auto& f : nrs_host::Masker::ParseFilters(in))
            std::printf("%s|%d|%s|%d %d %d %d %d|%s\n", argv[a], f.kind, f.name.c_str(), f.p[0], f.p[1], f.p[2], f.p[3], f.p[4], f.path.c_str());
    }
    return 0;
}
"""


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
    # the record the binding hands over has the header's layout: kind, five ints, pointer, three ints
    assert C.sizeof(nrs.FrontFilter) == 48 and nrs.FrontFilter.mask.offset == 24 and nrs.FrontFilter.w.offset == 32
    assert (nrs.FRONT_BRIGHT, nrs.FRONT_BORDER, nrs.FRONT_PREDEFINED) == (0, 1, 2) and (nrs.FRONT_GRAY, nrs.FRONT_CLAHE) == (0, 1)
    for text in ("NRS_FRONT_BRIGHT = 0, NRS_FRONT_BORDER = 1, NRS_FRONT_PREDEFINED = 2", "NRS_FRONT_IMAGE_GRAY = 0, NRS_FRONT_IMAGE_CLAHE = 1",
                 "#define NRS_FRONT_MAX_FILTERS 8"):
        assert text in hdr


def _python_parse(path):
    """masker.cc:32-69 once more: first word names the filter, the rest are its arguments"""
    out = []
    for line in open(path).read().split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "BorderFilter":
            out.append((1, "BorderFilter", [int(v) for v in t[1:6]], ""))
        elif t[0] == "BrightFilter":
            out.append((0, "BrightFilter", [int(t[1]), 0, 0, 0, 0], ""))
        elif t[0] == "Predefined":
            out.append((2, "PredefinedFilter", [0] * 5, t[1]))
    return out


def test_masker_mirror_parses_the_filter_files(tmp_path):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "filters", "*.filters.txt")))
    assert len(files) >= 5
    extra = tmp_path / "odd.filters.txt"                        # unknown names and blank lines are skipped, CRLF-free last line without newline
    extra.write_text("# comment\n\nSomethingElse 1 2\nBorderFilter 1 2 3 4 5\nBrightFilter 17")
    files.append(str(extra))
    src, exe = tmp_path / "parse_filters.cpp", tmp_path / "parse_filters"
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nr-slam_amd", "host"),
                           str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)] + files, text=True).splitlines():
        path, kind, name, p, arg = line.split("|")
        got.setdefault(path, []).append((int(kind), name, [int(v) for v in p.split()], arg))
    for path in files:
        assert got.get(path, []) == _python_parse(path), path
    by_name = {os.path.basename(p).split(".")[0]: got[p] for p in files}
    assert by_name["endomapper"] == [(0, "BrightFilter", [225, 0, 0, 0, 0], ""), (2, "PredefinedFilter", [0] * 5, "./data/endomapper/endoscopy_borders.png")]
    assert by_name["hamlyn_01"] == [(0, "BrightFilter", [255, 0, 0, 0, 0], "")]
    assert by_name["hamlyn_19"] == [(0, "BrightFilter", [200, 0, 0, 0, 0], ""), (1, "BorderFilter", [20, 20, 50, 20, 0], "")]
    assert by_name["odd"] == [(1, "BorderFilter", [1, 2, 3, 4, 5], ""), (0, "BrightFilter", [17, 0, 0, 0, 0], "")]


def test_front_oracle_shares_nothing_with_the_library():
    """the yardstick imports NumPy only"""
    src = open(os.path.join(ROOT, "tests", "front_oracle.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", src, re.M) == ["numpy"]
