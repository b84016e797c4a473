#!/usr/bin/env python3
"""Is the device code of pcrcg_amd/csrc the same as at another git revision?  The check for a host-side refactor.

    python scripts/compare_device_code.py REV [file.hip ...]      (default: every .hip file of pcrcg_amd/csrc)

Each file is compiled twice, from REV (`git archive` into a temporary directory) and from the working tree, each with the
flags its own tree's Makefile gives the file (EXACT_SRC there: -ffp-contract=off) plus `-S --cuda-device-only`.  Lines
that contain `__hip_cuid_` (a hash of the source text) are dropped; the two assembly files must then be byte-identical, kernel order included (a file whose template instances come
out in another order fails here and needs a comparison per symbol by hand).  Exit status 0: every file identical.
"""
import concurrent.futures
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def exact_sources(root):
    """The files a tree compiles with -ffp-contract=off: EXACT_SRC of ITS Makefile."""
    with open(os.path.join(root, "pcrcg_amd", "csrc", "Makefile")) as f:
        for ln in f:
            if ln.startswith("EXACT_SRC"):
                return set(ln.split(":=", 1)[1].split())
    sys.exit("no EXACT_SRC in the Makefile of " + root)


def assembly(root, src, out):
    csrc = os.path.join(root, "pcrcg_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(root, "include"), "-I" + csrc]
    if src in exact_sources(root):
        cmd.append("-ffp-contract=off")
    cmd += ["-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def compare(rev_root, src, tmp):
    old = assembly(rev_root, src, os.path.join(tmp, "old_" + src + ".s"))
    new = assembly(REPO, src, os.path.join(tmp, "new_" + src + ".s"))
    kernels = sum(1 for ln in new if ".amdhsa_kernel " in ln)
    if old == new:
        return src, True, "identical (%d lines, %d kernels)" % (len(new), kernels)
    first = next((i for i, (x, y) in enumerate(zip(old, new)) if x != y), min(len(old), len(new)))
    return src, False, "DIFFERS: %d vs %d lines, first at line %d: %r / %r" % (len(old), len(new), first + 1, "".join(old[first:first + 1]),
                                                                             "".join(new[first:first + 1]))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    csrc = os.path.join(REPO, "pcrcg_amd", "csrc")
    files = sys.argv[2:] or sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp:
        rev_root = os.path.join(tmp, "rev")
        os.makedirs(rev_root)
        tar = subprocess.run(["git", "-C", REPO, "archive", rev, "pcrcg_amd/csrc", "include"], check=True, stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", rev_root], input=tar.stdout, check=True)
        jobs = int(os.environ.get("MAX_JOBS", "8"))
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            results = list(pool.map(lambda f: compare(rev_root, f, tmp), files))
    ok = True
    for src, same, msg in results:
        print("%-20s %s" % (src, msg))
        ok = ok and same
    print("device code %s %s" % ("identical to" if ok else "DIFFERS from", rev))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
