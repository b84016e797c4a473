"""Writes tests/golden/indoor_frames.npz: the seeded frames of tests/indoor_ref.golden_inputs and their Image.NEAREST
resizes BY PIL ITSELF (Image.fromarray(...).resize((width, height), Image.NEAREST)) -- 7x11 -> 3x4 and 48x64 -> 12x16 for
16-bit depth, 48x64x3 -> 24x32 for colour -- so that the fixture is PIL's output and not the restatement's.  Needs PIL.

    python scripts/make_golden_indoor.py
"""
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import indoor_ref as IR  # noqa: E402


def pil_resize(frame, size):
    return np.asarray(Image.fromarray(frame).resize((size[1], size[0]), Image.NEAREST))


def main():
    out = {}
    for name, frames in IR.golden_inputs().items():
        out[name] = frames
        out[name + "_resized"] = np.stack([pil_resize(f, IR.GOLDEN_SIZES[name]) for f in frames]).astype(frames.dtype)
        assert out[name + "_resized"].shape[1:3] == IR.GOLDEN_SIZES[name]
    for v in (0, 1, 32767, 32768, 65535):
        assert any((out[k] == v).any() for k in ("depth_odd_resized", "depth_big_resized")), v
    assert (out["color_resized"] == 0).any() and (out["color_resized"] == 255).any()
    path = os.path.join(REPO, "tests", "golden", IR.GOLDEN)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
