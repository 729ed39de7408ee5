"""Tests of eval_config.coco_eval_options and the device match of the COCO evaluator (mtlssl_coco_match)."""
