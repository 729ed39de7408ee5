"""Helpers shared by the float64 kernel tests (test_gpu_head_kernels.py, test_gpu_spatial_kernels.py,
test_gpu_option_kernels.py): elementwise comparison against a float64 reference with a per-element bound, bitwise
comparison, host <-> device copies.
A plain module: no fixtures, not a conftest."""
import numpy as np
import torch

EPS = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float32).tiny)
f32 = np.float32


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def host(t):
    return t.cpu().numpy()


def within(got, ref, tol, what):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err - tol, -np.inf))), err.shape) if err.ndim else ()
        raise AssertionError("%s: %d elements out of bound; worst at %s: got %r, float64 %r, bound %r"
                             % (what, int(bad.sum()), i, got[i], ref[i], np.broadcast_to(tol, err.shape)[i]))


def bits(a, b, what):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    diff = a.view(np.int32) != b.view(np.int32)
    assert not diff.any(), "%s: %d elements differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), np.argwhere(diff)[0], a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])
