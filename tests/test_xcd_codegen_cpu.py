"""The register budget of the XCD-resident chunk kernel (`k_train_chunk_xcd`, csrc/step_xcd.hip), read from the AMDGPU metadata
of a device-only compile with the flags of ggad_amd/build.py.  The kernel is bound by dependent memory round trips;
a spilled loop-invariant address is reloaded inside the step loop behind a full wait, i.e. is one more round trip on the critical
path of every step.  So: the two compile-time-width instances (D = 64, the trained width) have no scratch at all, the two
run-time-width instances no more than before this test existed (184 / 192 bytes per lane), all four at 2 waves per SIMD (eight
waves per workgroup on the four SIMDs of a compute unit).  Metadata fields only; scripts/xcd_codegen_report.py prints them."""
import importlib.util
import os
import re
import shutil

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

PRIVATE_BYTES_MAX = {"<1,64>": 0, "<2,64>": 0, "<1,0>": 184, "<2,0>": 192}


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("xcd_codegen_report", os.path.join(ROOT, "scripts", "xcd_codegen_report.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    tmp_path = tmp_path_factory.mktemp("xcd_codegen")
    asm = rep.compile_asm(os.path.join(ROOT, "ggad_amd", "csrc", "step_xcd.hip"), str(tmp_path))
    meta = rep.kernel_metadata(open(asm).read())
    out = {}
    for name, m in meta.items():
        if rep.KERNEL in name:
            mode, width = re.search(r"ILi(\d+)ELi(\d+)E", name).groups()      # template arguments <MODE, DT> of the mangled name
            out[f"<{mode},{width}>"] = (m, rep.waves_per_simd(m))
    return out


def test_all_four_instances_are_compiled(instances):
    assert sorted(instances) == sorted(PRIVATE_BYTES_MAX), sorted(instances)


@pytest.mark.parametrize("inst", sorted(PRIVATE_BYTES_MAX))
def test_private_segment_and_occupancy(instances, inst):
    m, waves = instances[inst]
    assert m[".private_segment_fixed_size"] <= PRIVATE_BYTES_MAX[inst], m
    if PRIVATE_BYTES_MAX[inst] == 0:
        assert m[".vgpr_spill_count"] == 0, m
    assert waves == 2, m
