"""xt_tuning.bwd_fuse21 on the C ABI: the field is in the header struct, in lib.Tuning and in get_tuning(); values outside
0..2 are refused; the default a fresh process reports is the one DESIGN.md section 0 states."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_tuning_fields():
    src = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    body = src[src.index("typedef struct xt_tuning {"):src.index("} xt_tuning;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"int32_t\s+(\w+)\s*;", body)


def test_knob_is_the_last_field_of_the_struct_on_both_sides_of_the_abi():
    from xingtian_amd import lib
    fields = _header_tuning_fields()
    assert fields[-1] == "bwd_fuse21"
    assert [n for n, _ in lib.Tuning._fields_] == fields
    assert "bwd_fuse21" in lib.get_tuning()
    assert lib.load().xt_abi_version() == 12        # appended under ABI 12


def test_values_outside_0_to_2_are_refused():
    from xingtian_amd import lib
    before = lib.get_tuning()
    try:
        for v in (0, 1, 2):
            lib.set_tuning(bwd_fuse21=v)
            assert lib.get_tuning()["bwd_fuse21"] == v
        for v in (3, -1):
            with pytest.raises(RuntimeError, match="bwd_fuse21"):
                lib.set_tuning(bwd_fuse21=v)
            assert lib.get_tuning()["bwd_fuse21"] == 2
    finally:
        lib.set_tuning(bwd_fuse21=before["bwd_fuse21"])
    assert lib.get_tuning() == before


def test_default_of_a_fresh_process_is_what_design_md_states():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec0 = design[design.index("## 0."):design.index("## 1.")]
    m = re.search(r"`bwd_fuse21`[^\n]*?default\s+\**(\d)\**", sec0)
    assert m, "DESIGN.md section 0 does not state the default of bwd_fuse21"
    out = subprocess.run([sys.executable, "-c", "from xingtian_amd import lib; print(lib.get_tuning()['bwd_fuse21'])"],
                         check=True, cwd=ROOT, capture_output=True, text=True).stdout.strip()
    assert int(out) == int(m.group(1))
