"""Cost of CocoDetectionEvaluator.evaluate() through the host match (nested numpy / Python loops per image, category,
area range and maxDets) and through the device match (ops.coco_match: one launch for every segment), on the same
evaluator contents.

    python tools/coco_eval_cost.py [--images N] [--out profiles/coco_eval_cost.json]

Synthetic contents: 80 classes, 100 detections per image, 7 groundtruth boxes per image (a tenth of them crowd). Class
concentration: every image draws 4 'present' classes; its groundtruth boxes and 90% of its detections fall on those,
the rest of the detections on any class — real detectors pile their 100 boxes onto the few classes of the picture,
which is what makes the host loops long. Detections are jittered groundtruth boxes or noise, scores uniform.

Without --images the host path is timed on 40 images first and the image count is scaled to about one minute of host
time (at most 5000, COCO val2017's size). One timed call of each path, wall time; the device path reports its table
build, kernel, copy back and accumulation separately (the kernel with a synchronisation on either side). Both results
must be equal, number for number."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES, DETECTIONS, GROUNDTRUTH, PRESENT, ON_PRESENT, CROWD = 80, 100, 7, 4, 0.9, 0.1


def contents(num_images, seed=0):
    import numpy as np
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(num_images):
        present = rng.choice(CLASSES, PRESENT, replace=False)
        yx = rng.uniform(0, 400, (GROUNDTRUTH, 2))
        gb = np.concatenate([yx, yx + rng.uniform(10, 240, (GROUNDTRUTH, 2))], 1)
        gc = present[rng.randint(0, PRESENT, GROUNDTRUTH)]
        src = rng.randint(0, GROUNDTRUTH, DETECTIONS)
        db = gb[src] + rng.uniform(-15, 15, (DETECTIONS, 4))
        near = rng.uniform(size=DETECTIONS) < 0.6
        dc = np.where(near, gc[src], present[rng.randint(0, PRESENT, DETECTIONS)])
        dc = np.where(rng.uniform(size=DETECTIONS) < ON_PRESENT, dc, rng.randint(0, CLASSES, DETECTIONS))
        out.append((gb, gc, rng.uniform(size=GROUNDTRUTH) < CROWD, db, rng.uniform(0, 1, DETECTIONS), dc))
    return out


def evaluator(images, device=None):
    from mtl_ssl_amd.evaluation import CocoDetectionEvaluator
    ev = CocoDetectionEvaluator(CLASSES, DETECTIONS, device=device)
    for i, (gb, gc, crowd, db, ds, dc) in enumerate(images):
        ev.add_single_ground_truth_image_info(i, gb, gc, crowd)
        ev.add_single_detected_image_info(i, db, ds, dc)
    return ev


def timed(ev):
    t0 = time.perf_counter()
    res = ev.evaluate()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_cost.json"))
    ap.add_argument("--images", type=int, default=0, help="0: as many as the host path evaluates in about a minute")
    ap.add_argument("--host_seconds", type=float, default=60.0)
    f = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.build()
    n, probe = f.images, None
    if not n:
        probe = timed(evaluator(contents(40)))[0]
        n = int(max(40, min(5000, 40 * f.host_seconds / probe)))
    images = contents(n)
    dev = evaluator(images, "cuda:0")
    timed(evaluator(contents(8), "cuda:0"))                       # warm-up: library load, first launch
    dev_s, dev_res = timed(dev)
    parts = dict(dev.timings)
    host_s, host_res = timed(evaluator(images))
    same = all((np.asarray(host_res[k]) == np.asarray(dev_res[k])).all() for k in ("stats", "per_class_ap", "per_class_stats"))
    res = {"note": "tools/coco_eval_cost.py on one MI355X, one run, wall time of one evaluate() call per path.",
           "device": torch.cuda.get_device_name(0), "images": n, "classes": CLASSES, "detections_per_image": DETECTIONS,
           "groundtruth_per_image": GROUNDTRUTH,
           "class_concentration": "%d present classes per image hold its groundtruth and %d%% of its detections"
                                  % (PRESENT, round(ON_PRESENT * 100)),
           "host_probe_40_images_s": probe,
           "host_path_s": host_s,
           "device_path_s": dev_s,
           "device_path_parts_s": {k: parts[k] for k in ("table_build_s", "kernel_s", "copy_s", "accumulate_s")},
           "results_equal": bool(same), "AP": float(dev_res["AP"])}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(f.out), exist_ok=True)
    with open(f.out, "w") as fh:
        json.dump(res, fh, indent=1)
    if not same:
        raise SystemExit("the device path and the host path disagree")


if __name__ == "__main__":
    main()
