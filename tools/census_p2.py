#!/usr/bin/env python3
"""Dynamic VALU instruction count of one Poseidon2 permutation from the gfx950 ISA.

Compiles tools/ubench_p2.hip (which inlines p2::permute once inside a loop) to assembly, splits
the kernel at its two rolled loops (four full rounds each, `#pragma unroll 1` in
poseidon2_core.hpp) and weights their bodies by the trip count.  The result is the constant
raiko_amd/segment.py:P2_VALU_PER_PERMUTATION used by bench.py's `roofline.alu`.

  python tools/census_p2.py                       (needs hipcc; no GPU)
  python tools/census_p2.py -D RK_P2_DIRECT       (the one-round-at-a-time partial rounds)
  python tools/census_p2.py -D RK_P2_BLOCK=2      (blocks of two partial rounds)
  python tools/census_p2.py --width 16            (SP1's instance, p2::Core<16, 13, 1>)
  python tools/census_p2.py -D RK_P2_EXT_M4_FIRST (the external layer with M4 per block first)
  python tools/census_p2.py --kernels             (what the flagship runs: the chained-block loop of hash_rows_kernel
                                                   and the body of hash_fold_kernel from kernels_hash.hip, four instances)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find_loops(lines):
    """(first, last) line index of every loop: a label that is the target of a backward branch"""
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(lines):
        m = re.search(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    return sorted(loops)


def count(lines, a, b):
    """VALU, plain add/sub among them, 64-bit register copies among them, and s_nop (not VALU: hazard padding)"""
    n = fast = mov64 = nop = 0
    for l in lines[a:b + 1]:
        t = l.strip().split(" ")[0] if l.strip() else ""
        if t.startswith("v_"):
            n += 1
            fast += bool(re.match(r"v_(add|sub|subrev)_u32", t))
            mov64 += t.startswith("v_mov_b64")
        nop += t == "s_nop"
    return n, fast, mov64, nop


def weighted(lines, region, inner, trips):
    """counts of `region` with the rolled loops `inner` (counted once in it) run trips[i] times"""
    total = list(count(lines, *region))
    for (a, b), n in zip(inner, trips):
        for i, c in enumerate(count(lines, a, b)):
            total[i] += (n - 1) * c
    return total


def report(name, lines, region, inner, trips):
    total = weighted(lines, region, inner, trips)
    print("%s: %d VALU (plain add/sub: %d) = %d + %s; v_mov_b64 %d; s_nop %d" %
          (name, total[0], total[1], total[0] - sum(n * count(lines, a, b)[0] for (a, b), n in zip(inner, trips)),
           " + ".join("%d x %d" % (n, count(lines, a, b)[0]) for (a, b), n in zip(inner, trips)), total[2], total[3]))


def kernels_mode(args, defs):
    """the permutations the flagship runs: the chained-block loop of hash_rows_kernel (zero-padding sponge) and the body
    of hash_fold_kernel, from the compiled kernels_hash.hip, per instance.  Each is split at its two rolled loops."""
    root = args.root
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "kh.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(root, "raiko_amd", "csrc")] + defs +
                              [os.path.join(root, "raiko_amd", "csrc", "kernels_hash.hip"), "-S", "--cuda-device-only", "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read().split("\n")
    trips = [int(x) for x in args.trips.split(",")]
    for w, rp in ((24, 21), (16, 13)):
        for m4 in (0, 1):
            core = "CoreILi%dELi%dELi%dEE" % (w, rp, m4)
            for kern in ("hash_rows_kernel", "hash_fold_kernel"):
                # the zero-padding instance of hash_rows_kernel (Lb0E) where the sponge kind is a template parameter
                heads = [i for i, l in enumerate(text) if re.match(r"^_Z\w*%s\w*%s\w*:" % (kern, core), l)]
                heads = [i for i in heads if "Lb1E" not in text[i]]
                assert len(heads) == 1, (kern, core, len(heads))
                start = heads[0]
                end = start + next(i for i, l in enumerate(text[start:]) if "s_endpgm" in l)
                lines = text[start:end]
                loops = find_loops(lines)
                name = "%s<%d, %d>" % (kern, w, m4)
                if kern == "hash_fold_kernel":
                    assert len(loops) == 2, loops
                    report(name + " body", lines, (0, len(lines) - 1), loops, trips)
                else:
                    # block loops: loops holding exactly two others; the chained-block loop that keeps the capacity
                    # comes first in both row endings
                    outer = [ab for ab in loops if sum(1 for cd in loops if cd != ab and ab[0] <= cd[0] and cd[1] <= ab[1]) == 2]
                    assert outer, loops
                    ab = outer[0]
                    inner = [cd for cd in loops if cd != ab and ab[0] <= cd[0] and cd[1] <= ab[1]]
                    report(name + " chained-block loop", lines, ab, inner, trips)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definition for the build")
    ap.add_argument("--width", type=int, choices=(24, 16), default=24)
    ap.add_argument("--kernels", action="store_true", help="count hash_rows_kernel's chained-block loop and hash_fold_kernel's body, all four instances")
    ap.add_argument("--trips", default="4,3", help="--kernels: trip counts of the two rolled loops (4,4 for a tree whose last full round is not peeled)")
    ap.add_argument("--root", default=ROOT, help="--kernels: the source tree to compile")
    args = ap.parse_args()
    defs = ["-D" + d for d in args.defines] + (["-DP2_UBENCH_W16"] if args.width == 16 else [])
    if args.kernels:
        return kernels_mode(args, ["-D" + d for d in args.defines])
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "p2.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "raiko_amd", "csrc")] + defs +
                              [os.path.join(ROOT, "tools", "ubench_p2.hip"), "-S", "--cuda-device-only", "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
    start = text.index("_Z6k_perm")
    lines = text[start:].split("\n")
    end = next(i for i, l in enumerate(lines) if "s_endpgm" in l)
    lines = lines[:end]
    # inner loops: nested in the harness loop
    loops = find_loops(lines)
    outer = max(loops, key=lambda ab: ab[1] - ab[0])
    inner = [ab for ab in loops if ab != outer and outer[0] <= ab[0] and ab[1] <= outer[1]]
    assert len(inner) == 2, loops

    total = weighted(lines, outer, inner, (4, 4))  # bodies run 4 times (rounds 0..3 and 4..7)
    print("VALU instructions per permutation: %d (plain add/sub: %d); loop bodies: %s" %
          (total[0], total[1], [count(lines, a, b)[0] for a, b in inner]))
    print("v_mov_b64 per permutation: %d; in the loop bodies: %s" % (total[2], [count(lines, a, b)[2] for a, b in inner]))
    print("s_nop per permutation: %d; in the loop bodies: %s" % (total[3], [count(lines, a, b)[3] for a, b in inner]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
