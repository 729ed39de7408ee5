"""mtlssl_draw_boxes (csrc/visualize.hip) bit for bit against a numpy restatement of its contract: outlines of
half-open integer boxes, painted in input order, clipped to the image, nothing else touched.

The module shares its name with tests/evaluation/test_gpu_postprocess.py on purpose: tests/conftest.py orders the GPU
suite by module name, and these run with the kernel-level stage."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
H, W = 37, 53                     # odd on purpose: a dense row is 159 bytes, no multiple of 4


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def draw_boxes_numpy(image, boxes, colors, thickness):
    out = image.copy()
    Hh, Ww = out.shape[:2]
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    for (y0, x0, y1, x1), c in zip(np.asarray(boxes, np.int64).reshape(-1, 4), colors):
        inside = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
        inner = (yy >= y0 + thickness) & (yy < y1 - thickness) & (xx >= x0 + thickness) & (xx < x1 - thickness)
        out[inside & ~inner] = c
    return out


def _image(rng, h=H, w=W):
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _run(image, boxes, colors, thickness):
    from mtl_ssl_amd import ops
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(image).to(dev)
    b = torch.from_numpy(np.asarray(boxes, np.int32).reshape(-1, 4)).to(dev)
    c = torch.from_numpy(np.asarray(colors, np.uint8).reshape(-1, 3)).to(dev)
    ops.draw_boxes(t, b, c, thickness)
    return t.cpu().numpy()


CASES = {
    "overlap": [[2, 3, 20, 30], [10, 15, 30, 45], [12, 17, 18, 28]],
    "clipped": [[-5, -7, 15, 20], [25, 40, 60, 90], [-100, -100, 200, 200], [-2 ** 31, 5, 2 ** 31 - 1, 9]],
    "degenerate": [[5, 5, 5, 30], [7, 9, 20, 9], [20, 30, 10, 10], [8, 8, 9, 9]],
    "thin": [[3, 3, 6, 40], [10, 10, 17, 17], [0, 0, H, W]],
}


@pytest.mark.parametrize("thickness", [1, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_draw_boxes_matches_numpy(case, thickness):
    rng = np.random.RandomState(3)
    image = _image(rng)
    boxes = np.asarray(CASES[case], np.int64)
    colors = rng.randint(0, 256, (len(boxes), 3)).astype(np.uint8)
    want = draw_boxes_numpy(image, boxes, colors, thickness)
    got = _run(image, boxes, colors, thickness)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    untouched = np.all(want == image, -1)
    assert np.array_equal(got[untouched], image[untouched])
    if case != "degenerate":
        assert not untouched.all()


@pytest.mark.parametrize("n", [0, 100])
def test_draw_boxes_counts(n):
    rng = np.random.RandomState(n)
    image = _image(rng)
    y0, x0 = rng.randint(-10, H, n), rng.randint(-10, W, n)
    boxes = np.stack([y0, x0, y0 + rng.randint(0, 30, n), x0 + rng.randint(0, 30, n)], 1).reshape(-1, 4)
    colors = rng.randint(0, 256, (n, 3)).astype(np.uint8)
    got = _run(image, boxes, colors, 2)
    assert np.array_equal(got, draw_boxes_numpy(image, boxes, colors, 2))
    if n == 0:
        assert np.array_equal(got, image)


def test_draw_boxes_into_a_column_slice_leaves_the_rest_of_the_rows_alone():
    """Rows 3 * 61 = 183 bytes apart, the painted image 53 pixels wide and starting one pixel in (byte offset 3)."""
    from mtl_ssl_amd import ops
    rng = np.random.RandomState(5)
    wide = _image(rng, H, 61)
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(wide).to(dev)
    boxes = np.asarray([[-3, -3, 20, 30], [10, 20, H + 5, W + 5]], np.int32)
    colors = np.asarray([[1, 2, 3], [250, 251, 252]], np.uint8)
    ops.draw_boxes(t[:, 1:1 + W], torch.from_numpy(boxes).to(dev), torch.from_numpy(colors).to(dev), 4)
    want = wide.copy()
    want[:, 1:1 + W] = draw_boxes_numpy(wide[:, 1:1 + W], boxes, colors, 4)
    assert np.array_equal(t.cpu().numpy(), want)


def test_draw_boxes_refuses_bad_arguments():
    from mtl_ssl_amd import lib, ops
    dev = torch.device("cuda", 0)
    t = torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev)
    b = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    c = torch.zeros((1, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(lib.MtlsslError):
        ops.draw_boxes(t, b, c, 0)
