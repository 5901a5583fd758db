"""Builds liblle_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def build_native(force=False, verbose=False):
    """liblle_hip.so (lle_amd/csrc), then the fourteen libraries linked against it: liblle_render.so (lle_amd/render: the renderer),
    liblle_shaping.so (lle_amd/shaping: reward shaping and laser-subgoal extras), liblle_coop.so (lle_amd/coop: cooperation edges
    and episode profiles), liblle_search.so (lle_amd/search: the exact shortest-plan search), liblle_forest.so (lle_amd/forest: that
    search over many maps at once), liblle_policy.so (lle_amd/policy: steps-to-go and expert actions of a whole batch),
    liblle_helpgraph.so (lle_amd/helpgraph: shortest plans under a restriction on who may help whom), liblle_trails.so
    (lle_amd/trails: shortest plans without a sequence of N help events), liblle_helpforest.so (lle_amd/helpforest: those two
    searches over many maps at once), liblle_cooptrails.so (lle_amd/cooptrails: the longest help trail of every environment's
    episode, over liblle_coop.so), liblle_cycles.so (lle_amd/cycles: shortest plans without a closed trail of help events over
    exactly N agents), liblle_cycleforest.so (lle_amd/cycleforest: that search over many maps at once), liblle_coopcycles.so
    (lle_amd/coopcycles: the closed help trails of every environment's episode, over liblle_coop.so and the logic of lle_amd/cycles)
    and liblle_policyforest.so (lle_amd/policyforest: steps-to-go tables of many maps at once and the lookup of a multi-map batch, over
    liblle_policy.so for the map fingerprint: the last entry of the list, which names the library it links against beside
    liblle_hip.so)."""
    for src, lib, *_over in (("csrc", "liblle_hip.so"), ("render", "liblle_render.so"), ("shaping", "liblle_shaping.so"), ("coop", "liblle_coop.so"),
                     ("search", "liblle_search.so"), ("forest", "liblle_forest.so"), ("policy", "liblle_policy.so"),
                     ("helpgraph", "liblle_helpgraph.so"), ("trails", "liblle_trails.so"), ("helpforest", "liblle_helpforest.so"),
                     ("cooptrails", "liblle_cooptrails.so"), ("cycles", "liblle_cycles.so"), ("cycleforest", "liblle_cycleforest.so"),
                     ("coopcycles", "liblle_coopcycles.so"), ("policyforest", "liblle_policyforest.so", "liblle_policy.so")):
        cmd = ["make", "-C", os.path.join(_HERE, src), "-j8"] + (["-B"] if force else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or res.returncode != 0:
            print(res.stdout)
        if res.returncode != 0:
            raise RuntimeError(f"building {lib} failed (hipcc --offload-arch=gfx950)")
    return os.path.join(_HERE, "liblle_hip.so")


def build_c_example(verbose=False, name="c_abi_rollout"):
    """examples/c_abi_rollout.c, examples/c_abi_multi_gpu.c: plain-C hosts over include/lle_hip.h and the HIP runtime (gcc, no
    torch, no Python)."""
    root = os.path.dirname(_HERE)
    src, out = os.path.join(root, "examples", name + ".c"), os.path.join(root, "examples", name)
    cmd = ["gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
           src, "-o", out, "-L" + _HERE, "-llle_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,$ORIGIN/../lle_amd", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError(f"building examples/{name} failed")
    return out
