"""GPU tests of the evaluator's multi-task metrics and eval-time NMS (python -m mtl_ssl_amd.eval end to end)."""
