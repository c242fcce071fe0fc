"""CPU (no GPU): the static audits of tests/test_isa_audit.py applied to the normals kernel (csrc/occ_normals.hip), and
its register budget: a one-wave kernel that runs two waves per SIMD beside anybody else must not spill."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_isa_audit import _asm  # noqa: E402
from rfdnet_amd.build import CODEGEN_FLAGS  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")
KERNEL = "occ_normals_kernel"


def test_normals_kernel_runs_at_equal_priority_and_uses_no_lds(tmp_path):
    """no s_setprio (test_no_kernel_runs_its_waves_at_unequal_priorities); no LDS at all, so the LDS-prologue audit
    (test_no_two_wave_kernel_runs_a_valu_prologue_on_lds_reads_into_mfma_code_without_a_barrier) has nothing to find --
    checked here as: no LDS allocation and no ds_ instruction but the cross-lane permutes of __shfl_xor"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_mfma_war
    asm = _asm(tmp_path, "occ_normals.hip", "occ_normals.s")
    text = open(asm).read()
    assert "s_setprio" not in text
    names = [n for n in re.findall(r"^(_Z\S*%s\S*):" % KERNEL, text, flags=re.M)]
    assert len(names) == 1, names
    st, problems = audit_mfma_war.audit(asm, KERNEL, min_mfma_gap=6, min_c_states=3)
    print("occ_normals.hip %s: %d MFMAs, %d loads, closest load to an MFMA source: %s MFMAs, findings %d"
          % (KERNEL, st['mfma'], st['loads'], st['min_ab_gap'], len(problems)))
    assert st['mfma'] > 0
    lds = [l for l in re.findall(r"^\s+(ds_\w+)", text, flags=re.M) if l not in ("ds_bpermute_b32", "ds_swizzle_b32")]
    assert lds == [], lds[:5]                    # (the cross-lane sums' ds_bpermute reads no LDS memory)
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", text)


def test_normals_kernel_register_budget(tmp_path):
    """-Rpass-analysis=kernel-resource-usage: two waves per SIMD, no VGPR spill, no scratch (SGPR spills go to VGPR lanes)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc] + CODEGEN_FLAGS + ["-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rfdnet_amd", "csrc"), "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "n.o"),
                        os.path.join(ROOT, "rfdnet_amd", "csrc", "occ_normals.hip")],
                       check=True, capture_output=True, text=True, cwd=str(tmp_path))
    rep = {}
    for k, v in re.findall(r"remark:\s+([A-Za-z/ \[\]]+?):\s+(\d+)", r.stderr):
        rep.setdefault(k.strip(), int(v))
    print("occ_normals_kernel:", rep)
    assert rep["VGPRs Spill"] == 0 and rep["ScratchSize [bytes/lane]"] == 0
    assert rep["Occupancy [waves/SIMD]"] >= 2 and rep["LDS Size [bytes/block]"] == 0
