"""Writes tests/golden/raster_isa_digests.json: SHA-256 of the device assembly of every k_raster instantiation but KIND_ANY and of
k_shade<PHONG> / k_shade<EYE>, one per function, comments and blank lines dropped (tests/test_user_shaders.py compares the build's
-save-temps assembly with them).  A basic-block label `.LBB<f>_<n>` carries the function's ordinal <f> in its file: it is read as
`.LBB_<n>`, where it is defined and where a branch names it, so that a kernel's digest does not depend on what else the file holds.

    python tests/golden/make_raster_isa_digests.py [path/to/kernels_raster-hip-amdgcn-amd-amdhsa-gfx950.s]

The digests pin these kernels to the instructions they had before user shaders were added, for the hipcc of the build.  Refresh
them only from a build whose kernels are known to be right (a new ROCm, or a deliberate change to k_raster / k_shade after the
GPU suite passed), and say so in the commit."""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = os.path.join(HERE, "..", "..", "tinyrenderder_amd", "csrc", "build", "kernels_raster-hip-amdgcn-amd-amdhsa-gfx950.s")


def functions(path):
    """{mangled name: [instruction lines]} of an amdgcn .s file, comments and blank lines dropped, block labels without the
    function's ordinal."""
    out, cur, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, buf = m.group(1), []
            continue
        if cur and line.startswith(".Lfunc_end"):
            out[cur] = buf
            cur = None
            continue
        if cur:
            s = line.split(";")[0].rstrip()
            if s:
                buf.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s) + "\n")
    return out


def digest(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def protected(name):
    """k_raster<KIND, ...> with KIND != 5 (KIND_ANY), k_shade<2> (PHONG), k_shade<3> (EYE)"""
    return ("k_raster" in name and "k_rasterILi5E" not in name) or "k_shadeILi2E" in name or "k_shadeILi3E" in name


if __name__ == "__main__":
    fs = functions(sys.argv[1] if len(sys.argv) > 1 else DEFAULT)
    with open(os.path.join(HERE, "raster_isa_digests.json"), "w") as f:
        json.dump({k: digest(v) for k, v in fs.items() if protected(k)}, f, indent=1, sort_keys=True)
