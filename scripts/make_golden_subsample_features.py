"""Generate tests/golden/subsample_features.npz: what the UNMODIFIED reference grid subsampling returns for points WITH
features and classes on the fixed cases of tests/subsample_ref.py (fixture_cases).

The reference's cpp_wrappers.zip is unpacked into a temporary directory; its grid_subsampling.cpp and cloud.cpp are
compiled there, with the flags of oracle/Makefile (the reference's distutils build: -std=c++11 -O2 -fwrapv
-D_GLIBCXX_USE_CXX11_ABI=0, no -march), together with the small driver below, which is this repository's own: it reads
one case from a binary file, calls grid_subsampling (entry "single") or batch_grid_subsampling (entry "batch") and writes
what came back.  Nothing compiled and nothing of the reference is kept: the fixture holds the outputs, and a checksum of
the inputs, which the tests rebuild from fixture_cases().

    python scripts/make_golden_subsample_features.py [path/to/cpp_wrappers.zip]

Runs only where the reference is present."""
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import subsample_ref as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "subsample_features.npz")
FLAGS = ["-std=c++11", "-O2", "-fwrapv", "-D_GLIBCXX_USE_CXX11_ABI=0", "-w"]

DRIVER = r"""
// in : int32 n, nb, fdim, ldim, max_p, single; float32 dl; int32 len[nb]; float32 pts[3n], feats[n*fdim]; int32 cls[n*ldim]
// out: int32 m; int32 out_len[nb]; float32 pts[3m], feats[m*fdim]; int32 cls[m*ldim]
#include "cpp_subsampling/grid_subsampling/grid_subsampling.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static void rd(FILE* f, T* p, size_t k) { if (k && fread(p, sizeof(T), k, f) != k) exit(2); }
template <typename T> static void wr(FILE* f, const T* p, size_t k) { if (k && fwrite(p, sizeof(T), k, f) != k) exit(3); }
int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 1;
    int h[6];
    float dl;
    rd(in, h, 6);
    rd(in, &dl, 1);
    const int n = h[0], nb = h[1], fdim = h[2], ldim = h[3], max_p = h[4], single = h[5];
    vector<int> len(nb), cls((size_t)n * ldim), s_cls, s_len;
    vector<float> xyz((size_t)n * 3), feats((size_t)n * fdim), s_feats;
    rd(in, len.data(), nb);
    rd(in, xyz.data(), xyz.size());
    rd(in, feats.data(), feats.size());
    rd(in, cls.data(), cls.size());
    fclose(in);
    vector<PointXYZ> pts(n), s_pts;
    for (int i = 0; i < n; ++i) pts[i] = PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    if (single) {
        grid_subsampling(pts, s_pts, feats, s_feats, cls, s_cls, dl, 0);
        s_len.push_back((int)s_pts.size());
    } else {
        batch_grid_subsampling(pts, s_pts, feats, s_feats, cls, s_cls, len, s_len, dl, max_p);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 1;
    const int m = (int)s_pts.size();
    if (s_feats.size() != (size_t)m * fdim || s_cls.size() != (size_t)m * ldim || (int)s_len.size() != nb) return 4;
    wr(out, &m, 1);
    wr(out, s_len.data(), nb);
    vector<float> o((size_t)m * 3);
    for (int i = 0; i < m; ++i) { o[3 * i] = s_pts[i].x; o[3 * i + 1] = s_pts[i].y; o[3 * i + 2] = s_pts[i].z; }
    wr(out, o.data(), o.size());
    wr(out, s_feats.data(), s_feats.size());
    wr(out, s_cls.data(), s_cls.size());
    fclose(out);
    return 0;
}
"""


def run_case(exe, tmp, case):
    n, nb = case["points"].shape[0], case["lengths"].shape[0]
    f, c = case["features"], case["classes"]
    fdim = 0 if f is None else f.reshape(n, -1).shape[1]
    ldim = 0 if c is None else c.reshape(n, -1).shape[1]
    src, dst = os.path.join(tmp, "case.in"), os.path.join(tmp, "case.out")
    with open(src, "wb") as fh:
        fh.write(np.array([n, nb, fdim, ldim, case["max_p"], int(case["entry"] == "single")], np.int32).tobytes())
        fh.write(np.float32(case["dl"]).tobytes())
        for a in (case["lengths"], case["points"], f, c):
            if a is not None:
                fh.write(a.tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    m = int(np.frombuffer(raw, np.int32, 1)[0])
    off = 4
    out = {}
    for key, dtype, count, shape in (("lengths", np.int32, nb, (nb,)), ("points", np.float32, 3 * m, (m, 3)),
                                     ("features", np.float32, m * fdim, (m, fdim)), ("classes", np.int32, m * ldim, (m, ldim))):
        out[key] = np.frombuffer(raw, dtype, count, off).reshape(shape).copy()
        off += count * 4
    assert off == len(raw)
    if f is None:
        del out["features"]
    if c is None:
        del out["classes"]
    return out


def main():
    ref_zip = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/cpp_wrappers.zip"
    if not os.path.exists(ref_zip):
        sys.exit("the reference's cpp_wrappers.zip is not here: " + ref_zip)
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        zipfile.ZipFile(ref_zip).extractall(tmp)
        root = os.path.join(tmp, "cpp_wrappers")
        with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
            fh.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + root, "-o", exe, os.path.join(tmp, "driver.cpp"),
                                                 os.path.join(root, "cpp_subsampling", "grid_subsampling", "grid_subsampling.cpp"),
                                                 os.path.join(root, "cpp_utils", "cloud", "cloud.cpp")])
        for case in R.fixture_cases():
            got = run_case(exe, tmp, case)
            store[case["name"] + "/checksum"] = np.array([R.input_checksum(case)], np.int64)
            for k, v in got.items():
                store[case["name"] + "/" + k] = v
            print("%-22s rows %5d  %s" % (case["name"], got["points"].shape[0], sorted(got)))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
