"""Writes tests/golden/smoke_variable_specs.json.gz: the VarSpecs (name, shape, trainable, weight decay, initialiser)
that model_builder.variable_specs yields for every smoke config, training and inference, in registration order — a
JSON object {"<config>:<mode>": [one line per variable]}, gzipped because it is 4 700 lines of generated text
(`python -c "import gzip; print(gzip.open(PATH, 'rt').read())"` shows it).

    python tests/golden/make_smoke_variable_specs.py [ROOT_OF_THE_TREE_TO_READ]

Run on the tree of the commit BEFORE a change that must leave those models alone (a checkout of it, given as the
argument); tests/batch_norm/test_host_model.py compares the current tree against the file."""
import glob
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = "smoke_variable_specs.json.gz"
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))


def load_golden():
    with gzip.open(os.path.join(HERE, GOLDEN), "rt") as f:
        return json.load(f)


def spec_lines(specs):
    return ["%s %s %d %r %r" % (s.name, "x".join(map(str, s.shape)), s.trainable, s.weight_decay, tuple(s.init))
            for s in specs]


def smoke_configs(root):
    return sorted(os.path.relpath(p, root).replace(os.sep, "/")
                  for pat in ("configs/smoke_*.config", "configs/vgg16/smoke_*.config")
                  for p in glob.glob(os.path.join(root, pat)))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from mtl_ssl_amd import config, model_builder
    out = {}
    for path in smoke_configs(ROOT):
        cfg = config.parse_pipeline_config(open(os.path.join(ROOT, path)).read())
        for mode, is_training in (("train", True), ("inference", False)):
            out["%s:%s" % (path, mode)] = spec_lines(model_builder.variable_specs(cfg.model, is_training))
    text = json.dumps(out, indent=0, sort_keys=True) + "\n"
    with open(os.path.join(HERE, GOLDEN), "wb") as raw:                 # mtime 0, no file name: the same bytes every time
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())
