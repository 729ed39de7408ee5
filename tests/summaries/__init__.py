"""GPU tests of the training / evaluation summaries: the variable-histogram kernel against its float64 restatement,
and the event files of trainer.train and python -m mtl_ssl_amd.eval end to end."""
