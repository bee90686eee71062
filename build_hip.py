"""Build the xaynet_amd._hip extension with hipcc for gfx950 (in-tree).

hipcc compiles both the device code (kernels.hip) and the pybind11 host
module in one shared object. No GPU is needed to build (cross-compile).
"""
import os
import subprocess
import sys
import sysconfig


def build(verbose=True, resource_usage=False):
    """resource_usage=True (`python build_hip.py --resource-usage`) rebuilds
    with -Rpass-analysis=kernel-resource-usage: the compiler then reports every
    kernel's registers, scratch and occupancy on stderr."""
    root = os.path.dirname(os.path.abspath(__file__))
    import pybind11

    src = [
        os.path.join(root, "xaynet_amd", "csrc", "gpu", "kernels.hip"),
        os.path.join(root, "xaynet_amd", "csrc", "gpu", "hip_bindings.cpp"),
    ]
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    out = os.path.join(root, "xaynet_amd", f"_hip{ext}")

    # skip if up to date (kernels.h: the C ABI both sources include)
    deps = src + [os.path.join(root, "xaynet_amd", "csrc", "gpu", h) for h in ("kernels.h", "limbs.h", "mask_quant.h", "model_codec.h", "u192.h", "unmask_round.h", "k1_candidates_lds_body.inc",
                        "k1_candidates_lds_u128_body.inc")]
    if not resource_usage and os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in deps):
        if verbose:
            print(f"_hip up to date: {out}")
        return out

    hipcc = "/opt/rocm/bin/hipcc"
    cmd = [
        hipcc,
        "--offload-arch=gfx950",
        "-O3",
        "-std=c++17",
        "-fPIC",
        "-shared",
        "-fvisibility=hidden",
        "-x", "hip", src[0],
        "-x", "hip", src[1],  # host-only file, but hipcc needs the HIP language mode
        f"-I{pybind11.get_include()}",
        f"-I{sysconfig.get_paths()['include']}",
        "-o", out,
    ]
    if resource_usage:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return out


if __name__ == "__main__":
    build(resource_usage="--resource-usage" in sys.argv[1:])
