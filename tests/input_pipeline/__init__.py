"""GPU tests of the asynchronous input pipeline (kernel, device batches, launchers)."""
