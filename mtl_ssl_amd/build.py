"""Build libmtlssl_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).

    python -m mtl_ssl_amd.build [--force]

Per-file flags: detection.hip is built with -ffp-contract=off so its float arithmetic is
evaluated in the same order as the CPU oracle (bit-exact integer outputs).
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libmtlssl_hip.so")
OBJ = os.path.join(HERE, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
SOURCES = {
    "detection.hip": ["-ffp-contract=off"],
    "ops.hip": ["-ffp-contract=off"],   # ROI max-pool arg-max must not flip on fma rounding
    "conv.hip": [],
    "glue.hip": ["-ffp-contract=off"],
    "depthwise.hip": [], "pool_concat.hip": [], "winograd.hip": [],
    "eval_metrics.hip": ["-ffp-contract=off"],   # evaluator NMS / edge-mask metric: numpy's double arithmetic
    "coco_eval.hip": ["-ffp-contract=off"],      # COCO match: the host evaluator's double IoU arithmetic
    "pascal_eval.hip": ["-ffp-contract=off"],    # PASCAL subset labelling: the host evaluator's double IoU arithmetic
    "aux_labels.hip": ["-ffp-contract=off"],     # labels from boxes: the host definitions' double arithmetic
    "summaries.hip": ["-ffp-contract=off"],      # variable histograms: the bucket rule and moments are double arithmetic
    # batch-statistics BatchNorm: the moving-average update is an unfused fp32 sequence, sqrt and division correctly rounded
    "batch_norm.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    "visualize.hip": [],              # box overlay of the evaluator's visualisations (integer work only)
    "comm.hip": [],                     # RCCL wrappers (host code only; RCCL itself is bound with dlopen)
}


def _digest(path, flags):
    h = hashlib.sha256()
    headers = sorted(os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith(".h"))      # every header there is
    for f in [path] + headers + [os.path.join(HERE, "..", "include", "mtlssl_hip.h")]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    jobs, digests = [], []
    for src, extra in SOURCES.items():
        path = os.path.join(CSRC, src)
        obj = os.path.join(OBJ, src + ".o")
        stamp = obj + ".sha"
        dig = _digest(path, COMMON + extra)
        digests.append(dig)
        if (not force and os.path.exists(obj) and os.path.exists(stamp)
                and open(stamp).read() == dig):
            continue
        jobs.append((path, obj, stamp, dig, extra))
    # the library records the digests it was linked from: a tree that carries the library without its object files
    # (a copy of a built tree) is up to date when they still match, and is not compiled again
    link_stamp = os.path.join(OBJ, "link.sha")
    link_dig = hashlib.sha256("\n".join(digests).encode()).hexdigest()
    if not force and os.path.exists(OUT) and os.path.exists(link_stamp) and open(link_stamp).read() == link_dig:
        return OUT

    def run(job):
        path, obj, stamp, dig, extra = job
        cmd = [HIPCC] + COMMON + extra + ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(stamp, "w") as f:
            f.write(dig)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if jobs or not os.path.exists(OUT):
        objs = [os.path.join(OBJ, s + ".o") for s in SOURCES]
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with open(link_stamp, "w") as f:
        f.write(link_dig)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
