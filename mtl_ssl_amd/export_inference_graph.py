"""Export launcher with the flags of object_detection/export_inference_graph.py:77-95: the variables of the model built
with is_training=False (exporter.py:390-409), restored from a trained checkpoint — with their moving averages when
eval_config.use_moving_averages is set (exporter.py:361-364) — written as a TensorFlow V2 checkpoint an inference
user loads with mtl_ssl_amd.inference.Detector.from_export.

    python -m mtl_ssl_amd.export_inference_graph --input_type image_tensor --pipeline_config_path path/to/pipeline.config \\
        --trained_checkpoint_prefix path/to/train_dir/model.ckpt --output_directory path/to/exported_model

The output directory (created if absent) holds
 - model.ckpt.index, model.ckpt.data-00000-of-00001: exactly the inference model's variables under the reference's
   names (no optimizer slots, no global step);
 - pipeline.config: the pipeline text as given;
 - export.json: input_type, the source checkpoint, whether moving averages were applied, the variable count.
frozen_inference_graph.pb and saved_model/ are TensorFlow graphs and are not written.

Runs on the host: the variable list comes from the model's constructors, no device buffer is allocated."""
import argparse
import json
import os
import sys

FORMAT_VERSION = 1
INPUT_TYPES = ("image_tensor", "encoded_image_string_tensor", "tf_example")      # exporter.py:177-182
NOT_WRITTEN = "frozen_inference_graph.pb and saved_model/ are not written: they are TensorFlow graphs"


def export_inference_graph(input_type, pipeline_config_path, trained_checkpoint_prefix, output_directory):
    """exporter.export_inference_graph on the checkpoint alone. Returns the export.json dict."""
    if input_type not in INPUT_TYPES:
        raise ValueError("Unknown input type: {}".format(input_type))            # exporter.py:341-342
    from . import checkpoint, config, model_builder, tf_checkpoint
    text = open(pipeline_config_path).read()
    cfg = config.parse_pipeline_config(text)
    use_ema = bool(cfg.get("eval_config", config.Msg("EvalConfig")).get("use_moving_averages", False))
    specs = model_builder.variable_specs(cfg.model, is_training=False)
    values, n_ema = checkpoint.inference_values(specs, trained_checkpoint_prefix, use_ema)
    os.makedirs(output_directory, exist_ok=True)
    tf_checkpoint.write_bundle(os.path.join(output_directory, "model.ckpt"), values)
    with open(os.path.join(output_directory, "pipeline.config"), "w") as fh:
        fh.write(text)
    meta = {"format_version": FORMAT_VERSION, "input_type": input_type,
            "trained_checkpoint_prefix": trained_checkpoint_prefix, "use_moving_averages": use_ema,
            "moving_averages_applied": n_ema, "num_variables": len(values)}
    with open(os.path.join(output_directory, "export.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    return meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input_type", default="image_tensor",
                    help="Type of input node. Can be one of [`image_tensor`, `encoded_image_string_tensor`, "
                         "`tf_example`]")
    ap.add_argument("--pipeline_config_path", default=None)
    ap.add_argument("--trained_checkpoint_prefix", default=None)
    ap.add_argument("--output_directory", default=None)
    f = ap.parse_args(sys.argv[1:] if argv is None else argv)
    # export_inference_graph.py:92-95
    if not f.pipeline_config_path:
        raise AssertionError("`pipeline_config_path` is missing")
    if not f.trained_checkpoint_prefix:
        raise AssertionError("`trained_checkpoint_prefix` is missing")
    if not f.output_directory:
        raise AssertionError("`output_directory` is missing")
    meta = export_inference_graph(f.input_type, f.pipeline_config_path, f.trained_checkpoint_prefix,
                                  f.output_directory)
    print(NOT_WRITTEN)
    print(json.dumps(meta))
    return meta


if __name__ == "__main__":
    main()
