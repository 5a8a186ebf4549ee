"""Regenerates tests/golden/interfaces_rs_lines.json from a raiko checkout: digests of the line fragments of
core/src/interfaces.rs, the file that provers/hip/patches/core-interfaces.patch applies to.  A fragment is a
whitespace-stripped line, or its tail from any whitespace-separated token on (`return x` -> `x`), each with and
without a trailing `;` or `,`; a digest is the first 16 hex digits of its SHA-256.  tests/test_ffi_crate.py checks
the patch's removed and context lines against them, so the test needs no raiko checkout.
usage: python tests/golden/make_interfaces_digests.py <raiko checkout>"""
import hashlib, json, os, re, sys
HERE = os.path.dirname(os.path.abspath(__file__))
REL = "core/src/interfaces.rs"


def digest(fragment):
    return hashlib.sha256(fragment.encode()).hexdigest()[:16]


def fragments(line):
    line = line.strip()
    if not line:
        return []
    out = []
    for s in [0] + [m.end() for m in re.finditer(r"\s+", line)]:
        tail = line[s:]
        out.append(tail)
        if tail[-1] in ";,":
            out.append(tail[:-1])
    return out


if __name__ == "__main__":
    raw = open(os.path.join(sys.argv[1], REL), "rb").read()
    lines = raw.decode().splitlines()
    out = {"file": REL, "file_sha256": hashlib.sha256(raw).hexdigest(), "n_lines": len(lines),
           "fragment_sha256_16": sorted({digest(f) for l in lines for f in fragments(l)})}
    json.dump(out, open(os.path.join(HERE, "interfaces_rs_lines.json"), "w"), indent=0)
