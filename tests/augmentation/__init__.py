"""GPU tests of the photometric augmentations of the input path (kernel, device batches, launchers)."""
