"""Register budget of the lane-split kernels (k_multi_step<..., LN = 2>), read from the code
objects of every specialised library build() produced: no private segment (no scratch, no SGPR
spill to memory) and at most 128 VGPRs, so that two waves per SIMD stay possible.  They exist for
the plain variant's four-way split with write-through stores only, once per observation dtype."""
import glob
import os
import re
import subprocess

import pytest

TOOLS = "/opt/rocm/lib/llvm/bin/"
# k_multi_step<M, LDS, OT, WT, DUP, XO, SP, POL, LN> in the Itanium mangling
NAME = re.compile(r"k_multi_stepILi(\d+)ELb([01])ELi(\d)ELb([01])ELb([01])ELi(\d)ELi(\d)ELb([01])ELi(\d)EE")
KERNEL = re.compile(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", re.S)


def test_lane_split_kernels_fit_the_register_budget(tmp_path):
    from gym_comm_amd import build, specialize
    if not all(os.path.exists(TOOLS + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    libs = sorted(glob.glob(os.path.join(specialize.SPEC_DIR, "*.so")))
    if not libs:
        pytest.skip("nothing built")
    for k, so in enumerate(libs):
        fat, co = str(tmp_path / ("f%d.bin" % k)), str(tmp_path / ("k%d.co" % k))
        subprocess.run([TOOLS + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
        subprocess.run([TOOLS + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
        notes = subprocess.run([TOOLS + "llvm-readelf", "--notes", co], capture_output=True, text=True,
                               check=True).stdout
        os.remove(fat), os.remove(co)
        fused = [(NAME.search(name), int(scratch), int(vgprs)) for name, scratch, vgprs in KERNEL.findall(notes)
                 if "k_multi_step" in name]
        assert fused and all(m for m, _, _ in fused), os.path.basename(so)
        split = [(m, s, v) for m, s, v in fused if m.group(9) != "1"]
        # one per observation dtype, all of them the plain four-way split, write-through
        assert sorted((m.group(9), m.group(3)) for m, _, _ in split) == \
            [("2", ot) for ot in "012"], os.path.basename(so)
        for m, scratch, vgprs in split:
            assert (m.group(2), m.group(4), m.group(6), m.group(7), m.group(8)) == ("0", "1", "0", "4", "0"), m.group(0)
            assert scratch == 0, (os.path.basename(so), m.group(0), scratch)
            assert vgprs <= 128, (os.path.basename(so), m.group(0), vgprs)
