"""The fold-in kernels (csrc/foldin_kernels.h) cross-compiled with the product's flags: no scratch, and no contraction --
the only v_fma_f64 are the ones of the correctly rounded fp64 division (between its v_div_scale_f64 pair and its
v_div_fixup_f64), so every other product and sum rounds on its own, as in the host solver the device restates."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myrrix-recommender_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("foldin_update_kernel", "foldin_solve_kernel", "foldin_anonymous_kernel", "foldin_estimate_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("foldin_isa")
    src = d / "foldin_only.hip"
    src.write_text('#include "%s"\n' % os.path.join(CSRC, "foldin_kernels.h"))
    out = d / "foldin_only.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", str(out), str(src)],
                   check=True, capture_output=True)
    return out.read_text()


def bodies(text):
    """{mangled kernel name: its instruction lines}"""
    out, name, cur = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if name and line.strip().startswith(".Lfunc_end"):
            name = None
        elif name:
            cur.append(line.strip())
    return out


def fma_outside_division(lines):
    """v_fma_f64 not inside a division sequence (a division: two v_div_scale_f64, then one v_div_fixup_f64; sequences
    may interleave)"""
    scales = fixups = bad = 0
    for l in lines:
        op = l.split()[0] if l else ""
        if op == "v_div_scale_f64":
            scales += 1
        elif op == "v_div_fixup_f64":
            fixups += 1
        elif op == "v_fma_f64" and scales <= 2 * fixups:
            bad += 1
    return bad


def test_no_scratch_and_no_contraction(asm):
    b = bodies(asm)
    for k in KERNELS:
        names = [n for n in b if k in n]
        assert names, k
        for n in names:
            assert not any(l.startswith("scratch_") for l in b[n]), n
            assert fma_outside_division(b[n]) == 0, n
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n){0,40}?\s+\.private_segment_fixed_size:\s+(\d+)", asm):
        if "foldin" in m.group(1):
            assert m.group(2) == "0", m.group(1)
    assert "v_mul_f64" in asm and "v_add_f64" in asm


def test_the_check_sees_a_contracted_product():
    lines = ["v_mul_f64 v[0:1], v[2:3], v[4:5]", "v_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]"]
    assert fma_outside_division(lines) == 1
    div = ["v_div_scale_f64 a", "v_div_scale_f64 b", "v_fma_f64 c", "v_div_fmas_f64 d", "v_div_fixup_f64 e"]
    assert fma_outside_division(div) == 0
