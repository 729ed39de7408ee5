"""GPU tests of checkpoint export and the Detector API (eval parity, exports, input types, mixed sizes)."""
