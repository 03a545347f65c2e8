#!/usr/bin/env python3
"""Device assembly of a level's specialised kernels + static instruction statistics per kernel.

    python tools/dump_isa.py open-divider_tomato 2 [--out /tmp/k.s] [--variant timeline]
                             [--structure] [--match k_multi_step] [--flags "-DX ..."] [--digest]

Compiles csrc/oc_kernels.hip (with the two headers it includes) exactly as specialize.ensure() would (-S --cuda-device-only instead
of -shared) and prints, for every kernel whose demangled name matches: VGPRs / SGPRs / scratch and
the static count of VALU / SALU / VMEM / SMEM / LDS / waitcnt / branch instructions.  Static counts of a
split kernel cover all arms; per-arm figures come from the `; %bb` ranges (use --arms).

--digest prints, for EVERY kernel, one line "<sha256 of its instruction stream and .amdhsa_*
descriptor block> <number of lines hashed>  <demangled name>", sorted by name: run it in two source trees and `diff` the
outputs to see whether a change touched any device code (comments, the per-build __hip_cuid_*
symbol and the .ident line do not enter the digest)."""
import argparse
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def classify(op):
    if op.startswith(("v_", "ds_bpermute")):
        return "VALU"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if op.startswith("s_waitcnt"):
        return "WAIT"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier", "s_setpc", "s_swappc")):
        return "CTRL"
    if op.startswith("s_nop"):
        return "NOP"
    if op.startswith("s_"):
        return "SALU"
    return "OTHER"


def kernel_digest(body, symbol=""):
    """sha256 over a kernel's labels + instructions and its .amdhsa_kernel descriptor block,
    comments and every other directive stripped (branch labels stay, without the index of the
    function in the module: .LBB<fn>_<n>, which only says in which order kernels were emitted; the
    kernel's own mangled name is replaced, so a kernel keeps its digest when its template gains an axis)"""
    lines = []
    code, _, rest = body.partition(".amdhsa_kernel")
    for ln in code.splitlines():
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())
        if symbol:          # (the kernel's own label: a new template axis renames it, the code is the same)
            ln = ln.replace(symbol, "<kernel>")
        if ln and (ln.startswith(".LBB_") or not ln.startswith(".")):
            lines.append(ln)
    for ln in rest.split(".end_amdhsa_kernel")[0].splitlines()[1:]:
        if ln.strip().startswith(".amdhsa_"):
            lines.append(" ".join(ln.split()))
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], len(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("level")
    ap.add_argument("agents", type=int)
    ap.add_argument("--out", default="/tmp/oc_isa.s")
    ap.add_argument("--variant", default="")
    ap.add_argument("--structure", action="store_true")
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--match", default="k_multi_step|k_step")
    ap.add_argument("--flags", default="")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    from gym_comm_amd import build, compiler, specialize
    lv = compiler.compile_level(a.level, a.agents, 500)
    hdr = a.out + ".spec.h"
    with open(hdr, "w") as f:
        f.write(specialize.spec_header_text(lv.blob, not a.structure))
    cmd = [build.hipcc_path(), "--offload-arch=" + build.ARCH]
    cmd += [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    if not a.generic:
        cmd += ["-DOC_SPECIALIZED", '-DOC_SPEC_FILE="%s"' % hdr] + ([] if a.structure else ["-DOC_SPEC_GEOMETRY"])
    cmd += specialize.VARIANT_FLAGS[a.variant] + a.flags.split()
    cmd += ["-S", "--cuda-device-only", "-o", a.out, os.path.join(build.CSRC, "oc_kernels.hip")]
    subprocess.run(cmd, check=True)
    text = open(a.out).read()
    # kernels: "<mangled>:" ... ".end_amdhsa_kernel" / s_endpgm region; split on .globl
    parts = re.split(r"\n\t\.globl\t(\S+)", text)
    rx = re.compile(a.match)
    if a.digest:
        rows = []
        for k in range(1, len(parts), 2):
            if ".amdhsa_kernel" not in parts[k + 1]:
                continue
            dem = subprocess.run(["c++filt", parts[k]], capture_output=True, text=True).stdout.strip()
            rows.append("%s %5d  %s" % (*kernel_digest(parts[k + 1], parts[k]), dem))
        print("\n".join(sorted(rows, key=lambda r: r.split("  ", 1)[1])))
        print("kernels:", len(rows))
        return
    for k in range(1, len(parts), 2):
        name, body = parts[k], parts[k + 1]
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if not rx.search(dem):
            continue
        code = body.split(".section\t.rodata")[0]
        counts = {}
        for ln in code.splitlines():
            m = re.match(r"\t([a-z_0-9]+)", ln)
            if m and not ln.startswith("\t."):
                c = classify(m.group(1))
                counts[c] = counts.get(c, 0) + 1
        meta = {key: re.search(r"; %s: (\d+)" % key, body) for key in ("NumVgprs", "NumSgprs", "ScratchSize", "Occupancy")}
        meta = {k2: (int(v.group(1)) if v else -1) for k2, v in meta.items()}
        short = re.sub(r"^void \(anonymous namespace\)::", "", dem)
        short = re.sub(r"\(.*$", "", short)
        print("%-64s vgpr %3d sgpr %3d scratch %d | %s | total %d" % (
            short, meta["NumVgprs"], meta["NumSgprs"], meta["ScratchSize"],
            " ".join("%s %d" % (c, counts.get(c, 0)) for c in ("VALU", "SALU", "VMEM", "SMEM", "LDS", "WAIT", "CTRL", "NOP")),
            sum(counts.values())))
    print("assembly:", a.out)


if __name__ == "__main__":
    main()
