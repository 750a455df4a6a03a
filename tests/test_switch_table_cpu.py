"""The debug / A-B switches: one table (nr-slam_amd/csrc/nrs_switches.hpp) holds the library's reads, the comment block of include/nrs.h,
README's paragraph and every name the tests, tools and the binding hand to the library together.  nrs_debug_set accepts any NRS_* name, so
a misspelt one in an A/B test would compare a launch form with itself and pass: here it fails.  Builds and runs host/ctx_check.cpp
(AddressSanitizer + UBSan; no GPU, no library) and reads its `--list`."""
import ast
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nr-slam_amd")
NAME = re.compile(r"NRS_[A-Z0-9_]*[A-Z0-9]")


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", PKG, "ctx_check"], check=True, capture_output=True, timeout=300)
    exe = os.path.join(PKG, "ctx_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ctx_check OK") and not r.stderr, r.stdout + r.stderr
    rows = [ln.split(None, 2) for ln in subprocess.run([exe, "--list"], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]
    assert len(rows) >= 71 and all(len(r) == 3 and r[1] in ("presence", "integer", "real") for r in rows)
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names)
    return set(names)


def _python_sources():
    files = glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
    files += glob.glob(os.path.join(PKG, "py", "*.py")) + [os.path.join(ROOT, "bench.py")]
    return sorted(f for f in files if os.path.abspath(f) != os.path.abspath(__file__))


def _is_environ(node):
    """os.environ / os.environ.get / os.getenv: a variable of the Python side (NRS_LIB, ...), not a switch handed to the library"""
    src = ast.unparse(node)
    return src.startswith("os.environ") or src.startswith("os.getenv")


def switch_names_used(path):
    """(name, line) of every NRS_* name a file uses as a switch: string constants that are a whole name or "NAME=value" -- the first argument
    of debug_set(...), keys of {...} dictionaries, members of tuples and lists of switches, parametrize cases -- and the keywords of
    dict(NRS_...=...).  Left out by USE, not by name: what the Python side looks up in os.environ itself, the values of a dictionary (the
    status names of the binding) and the match= pattern of pytest.raises."""
    tree = ast.parse(open(path).read(), path)
    skip = set()
    used = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call):
            if _is_environ(node.func):
                skip.update(id(a) for a in node.args)
            skip.update(id(k.value) for k in node.keywords if k.arg == "match")
            if isinstance(node.func, ast.Name) and node.func.id == "dict":
                used += [(k.arg, node.lineno) for k in node.keywords if k.arg and k.arg.startswith("NRS_")]
        elif isinstance(node, ast.Subscript) and _is_environ(node.value):
            skip.add(id(node.slice))
        elif isinstance(node, ast.Dict):
            skip.update(id(v) for v in node.values)
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and id(node) not in skip:
            m = re.fullmatch(r"(NRS_[A-Z0-9_]+)(=\S*)?", node.value)
            if m:
                used.append((m.group(1), node.lineno))
    return used


def test_every_switch_name_in_tests_tools_and_binding_is_a_row(table):
    used = [(n, os.path.relpath(f, ROOT), ln) for f in _python_sources() for n, ln in switch_names_used(f)]
    assert len({n for n, _, _ in used}) >= 45                       # (the scan sees the suite's switches at all)
    assert {"NRS_HOST_PACK", "NRS_NO_REARM", "NRS_RC", "NRS_SPEC_TRIALS"} <= {n for n, _, _ in used}   # debug_set(...), dict(...), "NAME=value", {...}
    unknown = [u for u in used if u[0] not in table]
    assert not unknown, "not in nrs_switches.hpp (a misspelt switch sets nothing): %s" % unknown


def test_the_scan_tells_switches_from_other_names(tmp_path):
    p = tmp_path / "sample.py"
    p.write_text('import os, pytest, nrs\n'
                 'nrs.debug_set("NRS_NO_LDSS", "1")\n'
                 'E = {"NRS_HEIR": "1"}\n'
                 'D = dict(NRS_SPEC_TRAILS=0)\n'
                 'for sw in ("NRS_HOST_WLAK", "1"), ("NRS_RC=7",): pass\n'
                 'L = os.environ.get("NRS_LIB"); M = os.environ["NRS_OTHER"]\n'
                 'S = {0: "NRS_OK"}\n'
                 'with pytest.raises(nrs.NrsError, match="NRS_ERR_NUMERIC"): pass\n')
    assert sorted(n for n, _ in switch_names_used(str(p))) == ["NRS_HEIR", "NRS_HOST_WLAK", "NRS_NO_LDSS", "NRS_RC", "NRS_SPEC_TRAILS"]


def test_header_block_names_the_table(table):
    text = open(os.path.join(ROOT, "include", "nrs.h")).read()
    a = text.index("---- Debug switches")
    block = text[a:text.index("int nrs_debug_set(", a)]
    assert "presence" in block                                       # (the header says which switches go by presence)
    assert set(NAME.findall(block)) == table | {"NRS_DEBUG"}


def test_readme_paragraph_names_rows_only(table):
    text = open(os.path.join(ROOT, "README.md")).read()
    a = text.index("**Debug switches**")
    para = text[a:text.index("\n\n", a)]
    names = set(NAME.findall(para))
    assert len(names) >= 50                                          # (the paragraph is found at all)
    assert names <= table | {"NRS_DEBUG"}, sorted(names - table)
