#!/usr/bin/env python3
"""What the device corner detection costs inside a VO frame: loam_vo_frame_stats.ms of one
loam_vo_frames_solve over `--pairs` frame pairs of `--width` x `--height` images, in detect mode
(detection + pyramids + tracking + the rest) and in images mode fed with the very corners the
detect mode produced (the rest alone).  The difference is the detection cost.  Prints one JSON line
and, with --out, writes it to a file.

    python tools/gftt_cost.py --pairs 128 --out profiles/gftt_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vloam-noted_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import lk_np  # noqa: E402  (the synthetic scene only)
from loam_amd import synth, vo  # noqa: E402
from loam_amd.depth import BatchDepth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--scenes", type=int, default=4, help="distinct image pairs, cycled over the frame pairs")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    rng = np.random.default_rng(0)
    g = BatchDepth(1)
    g.input(0, synth.frame(21, 4, 800)[0])
    g.process()
    scenes = []
    for s in range(a.scenes):
        sc = lk_np.Scene(100 + s, flat=(300.0, 200.0, 340.0, 240.0))
        shift = rng.uniform(-3.0, 3.0, 2)
        scenes.append((sc.render(a.width, a.height), sc.render(a.width, a.height, t=shift)))

    detect = vo.VOFrames(g, a.pairs, max_keypoints=1024)
    detect.enable_images(a.width, a.height)
    detect.enable_detection()
    images = vo.VOFrames(g, a.pairs, max_keypoints=1024)
    images.enable_images(a.width, a.height)
    ms = {"detect": [], "images": []}
    corners = 0
    for _ in range(a.repeats + 1):  # the first round warms up and is dropped
        for p in range(a.pairs):
            detect.input_image_pair(p, *scenes[p % a.scenes], 0, 0)
        detect.solve()
        ms["detect"].append(detect.result(0)[2].ms)
        corners = 0
        for p in range(a.pairs):
            pts = detect.tracks(p)[0]
            images.input_images(p, *scenes[p % a.scenes], pts, 0)
            corners += len(pts)
        images.solve()
        ms["images"].append(images.result(0)[2].ms)
        for p in (0, a.pairs - 1):  # the two modes computed the same frame
            assert np.array_equal(detect.result(p)[0], images.result(p)[0])
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    n_img = max(a.pairs, 1)
    rec = {"what": "loam_vo_frame_stats.ms of one loam_vo_frames_solve, detect mode beside images mode on the same "
                   "corners; gftt_ms is the difference of the medians",
           "pairs": a.pairs, "width": a.width, "height": a.height, "repeats": a.repeats,
           "corners_per_image": corners / n_img,
           "detect_ms": [round(v, 4) for v in ms["detect"][1:]], "images_ms": [round(v, 4) for v in ms["images"][1:]],
           "detect_ms_median": round(med["detect"], 4), "images_ms_median": round(med["images"], 4),
           "gftt_ms": round(med["detect"] - med["images"], 4),
           "gftt_ms_per_image": round((med["detect"] - med["images"]) / n_img, 4),
           # compulsory traffic: the image read, the eigenvalue plane written and read again
           "roofline_bytes": n_img * a.width * a.height * 9}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
