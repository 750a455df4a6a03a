"""CPU: nrs_options.sharded_kft (include/nrs.h) -- the struct grew at its end and the default keeps today's behaviour."""
import ctypes as C
import os
import re

import nrs

HERE = os.path.dirname(os.path.abspath(__file__))


def test_options_grew_at_the_end_with_sharded_kft():
    names = [f for f, _ in nrs.Options._fields_]
    assert names[-2:] == ["embedded_solver", "sharded_kft"]
    assert nrs.Options.sharded_kft.offset == nrs.Options.embedded_solver.offset + 4
    assert C.sizeof(nrs.Options) == (nrs.Options.sharded_kft.offset + 4 + 7) // 8 * 8


def test_header_declares_sharded_kft_last():
    src = open(os.path.join(HERE, "..", "include", "nrs.h")).read()
    body = src[src.index("typedef struct {\n    int32_t device;"):src.index("} nrs_options;")]
    fields = re.findall(r"^\s+(?:int32_t|uint32_t|double)\s+(\w+);", body, re.M)
    assert fields[-2:] == ["embedded_solver", "sharded_kft"]


def test_options_init_leaves_sharded_kft_off():
    lib = nrs.load_library()
    o = nrs.Options()
    o.sharded_kft = 7
    lib.nrs_options_init(C.byref(o))
    assert o.sharded_kft == 0 and o.embedded_solver == 0 and o.struct_size == C.sizeof(nrs.Options)
