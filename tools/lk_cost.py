#!/usr/bin/env python3
"""What the device Lucas-Kanade stage costs inside a VO frame: loam_vo_frame_stats.ms of one
loam_vo_frames_solve over `--pairs` frame pairs of `--points` points on `--width` x `--height`
images, in images mode (pyramids + tracking + the rest) and in tracks mode fed with the very tracks
the images mode produced (the rest alone).  The difference is the LK cost.  Prints one JSON line
and, with --out, writes it to a file.

    python tools/lk_cost.py --pairs 128 --points 1024 --out profiles/lk_cost.json
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
    ap.add_argument("--points", type=int, default=1024)
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
    pts = [np.stack([rng.uniform(0, a.width, a.points), rng.uniform(0, a.height, a.points)], axis=1)
           .astype(np.float32) for _ in range(a.pairs)]

    images = vo.VOFrames(g, a.pairs, max_keypoints=max(a.points, 1))
    images.enable_images(a.width, a.height)
    tracks = vo.VOFrames(g, a.pairs, max_keypoints=max(a.points, 1))
    ms = {"images": [], "tracks": []}
    tracked = 0
    for _ in range(a.repeats + 1):  # the first round warms up and is dropped
        for p in range(a.pairs):
            images.input_images(p, *scenes[p % a.scenes], pts[p], 0)
        images.solve()
        ms["images"].append(images.result(0)[2].ms)
        tracked = 0
        for p in range(a.pairs):
            prev, curr, status, _ = images.tracks(p)
            tracks.input_tracks(p, prev, curr, status, 0)
            tracked += int((status == 1).sum())
        tracks.solve()
        ms["tracks"].append(tracks.result(0)[2].ms)
        for p in (0, a.pairs - 1):  # the two modes computed the same frame
            assert np.array_equal(images.result(p)[0], tracks.result(p)[0])
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    rec = {"what": "loam_vo_frame_stats.ms of one loam_vo_frames_solve, images mode beside tracks mode on the same "
                   "tracks; lk_ms is the difference of the medians",
           "pairs": a.pairs, "points": a.points, "width": a.width, "height": a.height, "repeats": a.repeats,
           "tracked_fraction": tracked / max(a.pairs * a.points, 1),
           "images_ms": [round(v, 4) for v in ms["images"][1:]], "tracks_ms": [round(v, 4) for v in ms["tracks"][1:]],
           "images_ms_median": round(med["images"], 4), "tracks_ms_median": round(med["tracks"], 4),
           "lk_ms": round(med["images"] - med["tracks"], 4),
           "lk_us_per_point": round(1e3 * (med["images"] - med["tracks"]) / max(a.pairs * a.points, 1), 4)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
