"""Cost of PascalSubsetEvaluator.evaluate() through the host loops (_tp_fp once per subset, image and class) and
through the device labelling (ops.pascal_match: one launch for every segment and subset), on the same evaluator
contents.

    python tools/pascal_subset_cost.py [--images N] [--out profiles/pascal_subset_cost.json]

Synthetic contents, VOC07-test sized: 4 952 images, 20 classes, 300 detections and 3 groundtruth boxes per image (a
fifth of them difficult), with S = 1 subset ('all') and S = 4 (all / small / medium / large by box area). Every image
draws 3 'present' classes; its groundtruth boxes and 80% of its detections fall on those, the rest of the detections on
any class. Detections are jittered groundtruth boxes or noise, scores uniform.

One timed call of each path per S, wall time; the device path reports its table build, kernel, copy back and
accumulation separately (the kernel with a synchronisation on either side). Both results must be equal, number for
number. There is no pass/fail threshold on the time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IMAGES, CLASSES, DETECTIONS, GROUNDTRUTH, PRESENT, ON_PRESENT, DIFFICULT = 4952, 20, 300, 3, 3, 0.8, 0.2
RANGES = {1: (("all", 0.0, float("inf")),),
          4: (("all", 0.0, float("inf")), ("small", 0.0, 32.0 ** 2), ("medium", 32.0 ** 2, 96.0 ** 2),
              ("large", 96.0 ** 2, float("inf")))}


def contents(num_images, ranges, seed=0):
    import numpy as np
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(num_images):
        present = rng.choice(CLASSES, PRESENT, replace=False)
        yx = rng.uniform(0, 400, (GROUNDTRUTH, 2))
        gb = np.concatenate([yx, yx + rng.uniform(10, 240, (GROUNDTRUTH, 2))], 1)
        gc = present[rng.randint(0, PRESENT, GROUNDTRUTH)]
        area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        gs = ["|".join(n for n, lo, hi in ranges if lo <= a < hi) for a in area]
        src = rng.randint(0, GROUNDTRUTH, DETECTIONS)
        db = gb[src] + rng.uniform(-15, 15, (DETECTIONS, 4))
        near = rng.uniform(size=DETECTIONS) < 0.6
        dc = np.where(near, gc[src], present[rng.randint(0, PRESENT, DETECTIONS)])
        dc = np.where(rng.uniform(size=DETECTIONS) < ON_PRESENT, dc, rng.randint(0, CLASSES, DETECTIONS))
        out.append((gb, gc, rng.uniform(size=GROUNDTRUTH) < DIFFICULT, gs, db, rng.uniform(0, 1, DETECTIONS), dc))
    return out


def evaluator(images, device=None):
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    ev = PascalSubsetEvaluator(CLASSES, device=device)
    for i, (gb, gc, gd, gs, db, ds, dc) in enumerate(images):
        ev.add_single_ground_truth_image_info(i, gb, gc, is_difficult=gd, subsets=gs)
        ev.add_single_detected_image_info(i, db, ds, dc)
    return ev


def timed(ev):
    t0 = time.perf_counter()
    res = ev.evaluate()
    return time.perf_counter() - t0, res


def equal(a, b):
    import numpy as np
    return a["subset_names"] == b["subset_names"] and all(
        np.array_equal(a["ap_per_class"][n], b["ap_per_class"][n], equal_nan=True) and a["mean_ap"][n] == b["mean_ap"][n]
        for n in a["subset_names"]) and np.array_equal(a["corloc_per_class"], b["corloc_per_class"], equal_nan=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pascal_subset_cost.json"))
    ap.add_argument("--images", type=int, default=IMAGES)
    f = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    timed(evaluator(contents(8, RANGES[4]), "cuda:0"))              # warm-up: library load, first launch
    runs, same = {}, True
    for S, ranges in sorted(RANGES.items()):
        images = contents(f.images, ranges)
        dev = evaluator(images, "cuda:0")
        dev_s, dev_res = timed(dev)
        parts = dict(dev.timings)
        host = evaluator(images)
        host_s, host_res = timed(host)
        ok = equal(host_res, dev_res)
        same = same and ok
        runs["S=%d" % S] = {
            "subsets": [n for n, _, _ in ranges], "host_path_s": host_s,
            "host_path_parts_s": {k: host.timings[k] for k in ("match_s", "accumulate_s")}, "device_path_s": dev_s,
            "device_path_parts_s": {k: parts[k] for k in ("table_build_s", "kernel_s", "copy_s", "accumulate_s")},
            "results_equal": bool(ok), "mean_ap": {n: float(v) for n, v in dev_res["mean_ap"].items()}}
    res = {"note": "tools/pascal_subset_cost.py on one MI355X, one run, wall time of one evaluate() call per path.",
           "device": torch.cuda.get_device_name(0), "images": f.images, "classes": CLASSES,
           "detections_per_image": DETECTIONS, "groundtruth_per_image": GROUNDTRUTH, "runs": runs}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
    with open(f.out, "w") as fh:
        json.dump(res, fh, indent=1)
    if not same:
        raise SystemExit("the device path and the host path disagree")


if __name__ == "__main__":
    main()
