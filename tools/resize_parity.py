"""tests/resize_ref.py (Pillow's bilinear ImagingResample restated) against PyTorch's CPU antialiased resize, per case of
resize_ref.CASES: the largest difference in grey levels and the share of pixels that differ, for the uint8 path on contiguous and
on channels_last input (separate code paths in PyTorch) and for the float32 path rounded to uint8; and the mean absolute
difference on a smooth image.  Prints the markdown table docs/parity_log.md records.  CPU only.

    python tools/resize_parity.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_ref as rr  # noqa: E402

PATHS = rr.PATHS
measure = rr.measure


def main():
    print(f"torch {torch.__version__}")
    print("| case | " + " | ".join(f"{p}: max, share" for p in PATHS) + " | smooth image, mean abs diff (" + ", ".join(PATHS) + ") |")
    print("|---|" + "---|" * (len(PATHS) + 1))
    for i, case in enumerate(rr.CASES):
        cells = []
        for p in PATHS:
            mx, share, _ = measure(i, case, p)
            cells.append(f"{mx}, {share:.6f}")
        sm = ", ".join(f"{measure(i, case, p, smooth=True)[2]:.4f}" for p in PATHS)
        print(f"| {case[0]} | " + " | ".join(cells) + f" | {sm} |")


if __name__ == "__main__":
    main()
