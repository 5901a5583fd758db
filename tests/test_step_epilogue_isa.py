"""The headline instantiation, step_kernel<4,4,6,true,3>, sums its counters without LDS: the wave sums of kernel_common.hpp are DPP row
operations plus v_readlane, so no `ds_bpermute_b32` (what __shfl_xor compiles to: an LDS round trip each, 42 of them behind the row loop
before) is left in its body.  Compiled like tests/test_hot_path_budget.py, which keeps guarding the size and the registers:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S lle_amd/csrc/step_mode6.hip

Cross-compiles that translation unit: no GPU needed, about twenty seconds."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lle_amd", "csrc")
KERNEL = "_ZN3lle11step_kernelILi4ELi4ELi6ELb1ELi3EEEvNS_9BatchPtrsENS_10LaunchArgsE"


def kernel_body(source, mangled):
    """The instructions of one kernel of the device assembly, comments stripped."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "device.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", source, "-o", asm],
                       cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    at = text.index("\n" + mangled + ":")
    block = text[at:text.index("\n\t.section", at)]
    return [re.sub(r";.*", "", ln).strip() for ln in block.splitlines()]


def test_headline_instantiation_sums_its_counters_without_lds():
    body = kernel_body(os.path.join(CSRC, "step_mode6.hip"), KERNEL)
    ops = [ln.split()[0] for ln in body if ln and not ln.endswith(":") and not ln.startswith(".")]
    assert "s_endpgm" in ops and len(ops) > 1000, len(ops)  # (the body was found)
    assert not [op for op in ops if op.startswith("ds_bpermute")], "a wave sum went back to __shfl_xor"
    # what the sums are made of instead: DPP adds inside the rows of 16, the four rows through v_readlane (two packed words, both copies of post_step)
    assert sum(op == "v_readlane_b32" for op in ops) >= 8
    assert any(re.search(r"row_mirror", ln) for ln in body) and any(re.search(r"row_half_mirror", ln) for ln in body)
