"""Writes the fixtures of the rectifier tests from the reference's calibration sample (data/calib): the camera-parameter XML as it is, and one
608 x 416 window of each raw 2048 x 1536 sensor image as uint8 together with its offset.  A window is an exact camera with cx -= x0, cy -= y0,
so the real-image tests need no resampling.  Needs Pillow to read the PNG files.

    python tests/golden/make_golden_rectify.py <reference>/data/calib
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
X0, Y0, W, H = 720, 560, 608, 416


def main(src: str) -> None:
    from PIL import Image
    shutil.copyfile(os.path.join(src, "1_01_camera_param_head.xml"), os.path.join(HERE, "calib_head.xml"))
    for side in ("left", "right"):
        img = np.asarray(Image.open(os.path.join(src, f"1_10_sensor_raw_{side}.png")).convert("RGB"))
        assert img.shape == (1536, 2048, 3) and img.dtype == np.uint8
        out = os.path.join(HERE, f"rectify_raw_{side}_window.npz")
        np.savez_compressed(out, image=np.ascontiguousarray(img[Y0:Y0 + H, X0:X0 + W]), offset=np.array([X0, Y0], dtype=np.int64),
                            full_size=np.array([2048, 1536], dtype=np.int64))
        print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
