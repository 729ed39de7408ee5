"""Cost of the variable histograms of a training summary on configs[1] (Faster R-CNN ResNet-101, every head on):
ParamStore.histograms() — one device pass per flat buffer and two small copies back — against the same quantity from a
D2H copy of both buffers and the numpy restatement (summaries.histogram_numpy per variable).

    python tools/variable_histograms_cost.py [--out profiles/variable_histograms_configs1.json]

10 calls after 2 warm-ups, HIP events around the device path (they include its copies back) and wall time for both."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = "configs/frcnn_resnet101_coco_mtl.config"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variable_histograms_configs1.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    f = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mtl_ssl_amd import config, model_builder, summaries
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, CONFIG)).read())
    ps = model_builder.build(cfg.model, True, "cuda", seed=0).ps
    frozen = [s for s in ps.specs if not s.trainable]

    def host_path():
        out = {}
        for buf, specs in ((ps.weights.cpu().numpy(), ps.trainable_specs), (ps.frozen.cpu().numpy(), frozen)):
            for s in specs:
                out[s.name] = summaries.histogram_numpy(buf[s.offset:s.offset + s.size])
        return out

    for _ in range(f.warmup):
        dev = ps.histograms()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(f.iters):
        dev = ps.histograms()
    e1.record()
    torch.cuda.synchronize()
    dev_wall = (time.perf_counter() - t0) / f.iters * 1e3
    dev_events = e0.elapsed_time(e1) / f.iters
    host = host_path()                                               # one warm-up, then one timed pass (seconds each)
    t0 = time.perf_counter()
    host = host_path()
    host_wall = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(dev[n][1], host[n][1]) and (dev[n][0][:3] == host[n][0][:3]).all() for n in host)
    res = {"note": "tools/variable_histograms_cost.py on one MI355X, one run. Initial weights of configs[1].",
           "config": CONFIG, "device": torch.cuda.get_device_name(0), "variables": len(ps.specs),
           "floats": int(sum(s.size for s in ps.specs)), "warmup": f.warmup, "iters": f.iters,
           "device_pass": {"ms_per_call_events": dev_events, "ms_per_call_wall": dev_wall},
           "d2h_plus_numpy": {"ms_per_call_wall": host_wall, "calls": 1},
           "counts_min_max_num_equal": bool(same)}
    print(json.dumps(res))
    with open(f.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
