#!/usr/bin/env python3
"""Static VALU instruction count of the fused NTT kernels (ntt_fused.hpp) from the gfx950 ISA.

Compiles raiko_amd/csrc/kernels_ntt.hip to assembly and counts, for the five fused kernels of the flagship
shapes, the VALU instructions of one workgroup pass.  The kernels are straight-line code and a lane handles 16
elements of its 2^14-element tile, so the static count is the count per lane-tile.  Classes follow the cost model of
profiles/r01_ubench_isa.txt: multiplies and mads, v_min (the conditional subtractions), plain 32-bit add/sub (the
only class that issues at twice the rate) and the rest.  The 64-bit address instructions (v_add_co / v_addc_co
pairs, v_lshl_add_u64, v_lshlrev_b64) are part of "other" and listed on their own: a global access whose base is
workgroup-uniform needs none of them.

  python tools/census_ntt.py                   (needs hipcc; no GPU)
  python tools/census_ntt.py --all             (every nf_* instance, not only the flagship's five)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the flagship's instances: 2^22-point LDE (4x expanding forward, G = 8) and 2^20-point interpolation (G = 6)
FLAGSHIP = ["nf_fwd_contig_kernel<0>", "nf_fwd_contig_kernel<1>", "nf_fwd_contig_kernel<2>", "nf_inv_contig_kernel",
            "nf_strided_kernel<true, 8>", "nf_strided_kernel<false, 6>"]

ADDR64 = re.compile(r"v_(add_co_u32|addc_co_u32|lshl_add_u64|lshlrev_b64)")


def classify(op):
    if re.match(r"v_(mul|mad)_", op):
        return "mul/mad"
    if re.match(r"v_min_", op):
        return "min"
    if re.match(r"v_(add|sub|subrev)_u32", op):
        return "add/sub"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true", help="every nf_* kernel instance")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definition for the build")
    args = ap.parse_args()
    csrc = os.path.join(ROOT, "raiko_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "ntt.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", csrc] + ["-D" + d for d in args.defines] +
                              [os.path.join(csrc, "kernels_ntt.hip"), "-S", "--cuda-device-only", "-o", asm], stderr=subprocess.DEVNULL)
        lines = open(asm).read().split("\n")
    # kernel bodies: from the symbol's label to s_endpgm
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w*nf_\w+):", l)] if m]
    names = subprocess.run(["c++filt"] + [s for _, s in starts], capture_output=True, text=True, check=True).stdout.split("\n")
    print("%-32s %6s %8s %6s %8s %6s | %s" % ("kernel", "VALU", "mul/mad", "min", "add/sub", "other", "64-bit address instructions"))
    for (i, _), full in zip(starts, names):
        name = re.sub(r"\(.*", "", full.replace("(anonymous namespace)::", "")).replace("void ", "")
        if not (args.all or name in FLAGSHIP) or "table" in name:
            continue
        cls = {"mul/mad": 0, "min": 0, "add/sub": 0, "other": 0}
        addr = {}
        for l in lines[i:]:
            if "s_endpgm" in l:
                break
            t = l.split()[0] if l.split() else ""
            if not t.startswith("v_"):
                continue
            cls[classify(t)] += 1
            m = ADDR64.match(t)
            if m:
                k = re.sub(r"_e(32|64)$", "", t)
                addr[k] = addr.get(k, 0) + 1
        print("%-32s %6d %8d %6d %8d %6d | %s" % (name, sum(cls.values()), cls["mul/mad"], cls["min"], cls["add/sub"], cls["other"],
                                                  ", ".join("%d %s" % (v, k) for k, v in sorted(addr.items())) or "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
