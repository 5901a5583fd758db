"""Register and code budget of the headline instantiation, step_kernel<4,4,6,true,3> (level 6: 4 agents, 3 sources, row heads): no
scratch, no more registers and no more code than before the hot / cold split of the kernels with row heads -- 94 VGPRs, 105 SGPRs
and 11 700 bytes, as the compiler reports them for

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S lle_amd/csrc/step_mode6.hip

(what the split reached: profiles/r19_hot_path.md).  Cross-compiles that translation unit: no GPU needed, about twenty seconds."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lle_amd", "csrc")
KERNEL = "_ZN3lle11step_kernelILi4ELi4ELi6ELb1ELi3EEEvNS_9BatchPtrsENS_10LaunchArgsE"


def kernel_record(source, mangled):
    """What the compiler prints behind one kernel of the device assembly: code bytes, SGPRs, VGPRs, scratch bytes per lane."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "device.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", source, "-o", asm],
                       cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    at = text.index("\n" + mangled + ":")
    block = text[at:text.index("\n; Occupancy:", at)]
    want = {"code": r"; codeLenInByte = (\d+)", "sgprs": r"; TotalNumSgprs: (\d+)", "vgprs": r"; NumVgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)"}
    return {k: int(re.search(p, block).group(1)) for k, p in want.items()}


def test_headline_instantiation_stays_within_its_budget():
    r = kernel_record(os.path.join(CSRC, "step_mode6.hip"), KERNEL)
    print("step_kernel<4,4,6,true,3>:", r)
    assert r["scratch"] == 0, r
    assert r["vgprs"] <= 94 and r["sgprs"] <= 105, r
    assert r["code"] <= 11700, r
