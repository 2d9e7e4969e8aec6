#!/usr/bin/env python3
"""What the device ORB stage costs inside a VO frame: loam_vo_frame_stats.ms of one
loam_vo_frames_solve over `--pairs` frame pairs of `--width` x `--height` images, in six
configurations whose differences isolate the kernels:

    match    the two images alone (detection on both, blur, filter, describe, match, the rest)
    given    the images and the corners the detector finds (blur, filter, describe, match, the rest)
    desc     the kept keypoints and their descriptors (match, the rest)
    blur     the images and no keypoints (blur, an empty frame)
    dropped  the images and the corners moved outside the border (blur, filter, an empty frame)
    empty    no descriptors (an empty frame)

    blur_stage_ms = blur - empty, filter_stage_ms = dropped - blur,
    describe_stage_ms = given - desc - (dropped - empty), orb_stage_ms = given - desc,
    detect_both_stage_ms = match - given

(`<configuration>_ms` are a configuration's samples, `<configuration>_ms_median` their median.)

Prints one JSON line and, with --out, writes it to a file.

    python tools/orb_cost.py --pairs 128 --out profiles/orb_cost.json
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

    def handle(detect, describe):
        vf = vo.VOFrames(g, a.pairs, max_keypoints=1024)
        if detect or describe:
            vf.enable_images(a.width, a.height)
        if detect:
            vf.enable_detection()
        if describe:
            vf.enable_description()
        return vf

    # the corners of both images of every scene, as the match mode detects them (a detect pair each)
    det = handle(True, False)
    corners = []
    for prev, curr in scenes:
        per = []
        for side in (0, 1):
            det.input_image_pair(0, prev, curr, side, 0)
            det.solve()
            per.append(det.tracks(0)[0].copy())
        corners.append(per)
    det.close()

    match, given, desc = handle(True, True), handle(False, True), handle(False, False)
    none = np.zeros((0, 2), np.float32)
    runs = {k: [] for k in ("match", "given", "desc", "blur", "dropped", "empty")}
    kept = 0
    for _ in range(a.repeats + 1):  # the first round warms up and is dropped
        for p in range(a.pairs):
            match.input_image_pair_match(p, *scenes[p % a.scenes], 0)
        match.solve()
        runs["match"].append(match.result(0)[2].ms)
        for p in range(a.pairs):
            given.input_images_keypoints(p, *scenes[p % a.scenes], *corners[p % a.scenes])
        given.solve()
        runs["given"].append(given.result(0)[2].ms)
        kept = 0
        for p in range(a.pairs):
            (k0, d0), (k1, d1) = given.descriptors(p, 0), given.descriptors(p, 1)
            desc.input_descriptors(p, k0, d0, k1, d1, 0)
            kept += len(k0) + len(k1)
        desc.solve()
        runs["desc"].append(desc.result(0)[2].ms)
        for p in (0, a.pairs - 1):  # the three computed the same frame
            assert np.array_equal(match.result(p)[0], given.result(p)[0])
            assert np.array_equal(match.result(p)[0], desc.result(p)[0])
        for p in range(a.pairs):
            given.input_images_keypoints(p, *scenes[p % a.scenes], none, none)
        given.solve()
        runs["blur"].append(given.result(0)[2].ms)
        for p in range(a.pairs):
            out = [c * np.float32([0.0, 1.0]) for c in corners[p % a.scenes]]  # x = 0: outside the border
            given.input_images_keypoints(p, *scenes[p % a.scenes], *out)
        given.solve()
        runs["dropped"].append(given.result(0)[2].ms)
        assert len(given.descriptors(0, 0)[0]) == 0
        for p in range(a.pairs):
            desc.input_descriptors(p, none, np.zeros((0, 32), np.uint8), none, np.zeros((0, 32), np.uint8), 0)
        desc.solve()
        runs["empty"].append(desc.result(0)[2].ms)
    med = {k: float(np.median(v[1:])) for k, v in runs.items()}
    n_img = 2 * max(a.pairs, 1)
    blur_ms, filter_ms = med["blur"] - med["empty"], med["dropped"] - med["blur"]
    describe_ms = med["given"] - med["desc"] - (med["dropped"] - med["empty"])
    rec = {"what": "loam_vo_frame_stats.ms of one loam_vo_frames_solve in six configurations (medians); the stage "
                   "costs are their differences (see the tool's text)",
           "pairs": a.pairs, "width": a.width, "height": a.height, "repeats": a.repeats,
           "corners_per_image": sum(len(c) for per in corners for c in per) / (2 * len(corners)),
           "kept_per_image": kept / n_img,
           **{k + "_ms": [round(v, 4) for v in runs[k][1:]] for k in runs},
           **{k + "_ms_median": round(v, 4) for k, v in med.items()},
           # the stages, as differences of the medians above
           "blur_stage_ms": round(blur_ms, 4), "filter_stage_ms": round(filter_ms, 4),
           "describe_stage_ms": round(describe_ms, 4), "orb_stage_ms": round(med["given"] - med["desc"], 4),
           "orb_stage_ms_per_image": round((med["given"] - med["desc"]) / n_img, 5),
           "detect_both_stage_ms": round(med["match"] - med["given"], 4),
           # compulsory traffic: the blur reads and writes each image once; a descriptor reads 512 bytes
           # of the blurred plane and writes 32
           "blur_bytes": n_img * a.width * a.height * 2, "describe_bytes": kept * 544}
    rec["blur_gb_per_s"] = round(rec["blur_bytes"] / max(blur_ms, 1e-6) / 1e6, 1)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
