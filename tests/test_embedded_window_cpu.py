"""The one-call embedded BA window (include/nrs.h nrs_dba_solve_window_embedded / nrs_dba_window_edges_embedded) is declared, exported and
bound; and the windows tests/test_gpu_embedded_window.py compares on are not vacuous (checked here, on the host lists, without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrs_dba_solve_window_embedded", "nrs_dba_window_edges_embedded")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(nrs_ctx\* ctx," % name, text, re.M), name


def test_library_exports_the_entry_points(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    for name in NEW:
        assert name in nrs.SYMBOLS and hasattr(lib, name), name
    assert lib.nrs_dba_solve_window_embedded(*([None] * 18)) == -1          # a null context fails cleanly, no device needed
    assert lib.nrs_dba_window_edges_embedded(*([None] * 14)) == -1


def test_context_has_the_methods(lib_built):
    nrs = lib_built
    assert callable(getattr(nrs.Context, "dba_solve_window_embedded")) and callable(getattr(nrs.Context, "dba_window_edges_embedded"))


def test_the_gpu_cases_are_not_vacuous(lib_built):
    """every window of the GPU test, in both neighbour forms: the conditions it asserts on the host lists before comparing"""
    import embedded_window_cases as W
    for case in W.CASES:
        for form in W.FORMS:
            p, flag, nb = W.window(case, form)
            W.check_not_vacuous(case, form, p, flag, nb, lib_built.dba_build_edges_embedded(p["kf_points"], flag, nb))
