"""The evaluation kernels on the GPU against their numpy restatements (tests/test_mtl_metrics.py):
mtlssl_eval_nms bit for bit (indices and fp32 scores; the Gaussian weight through oracle/portable_math.py) over random
segments of every size up to the LDS bound, every type and both caps; mtlssl_edgemask_agreement's count for up- and
down-scaling at non-integer ratios; the bound error.

Named after tests/test_gpu_postprocess.py on purpose: tests/conftest.py orders the GPU suite by module name, and these
kernel-parity tests run with the kernel stage."""
import numpy as np
import pytest
import torch

from tests.test_mtl_metrics import edgemask_labels_numpy, eval_nms_numpy, portable_exp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _segment(rng, n):
    c = rng.uniform(0.2, 0.8, (max(1, n // 6), 2))
    c = c[rng.randint(0, len(c), n)] + rng.normal(0, 0.04, (n, 2))
    hw = rng.uniform(0.05, 0.3, (n, 2))
    boxes = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32)
    scores = rng.uniform(0.001, 1.0, n).astype(np.float32)
    if n > 3:
        scores[1] = scores[3]                   # one tie: the later input sorts first on both sides
    return boxes, scores


@pytest.mark.parametrize("nms_type", ["standard", "soft-linear", "soft-gaussian"])
@pytest.mark.parametrize("thr,sigma,cap", [(0.5, 0.5, 10000), (0.7, 0.3, 256), (0.3, 1.0, 7), (1.0, 0.5, 256)])
def test_eval_nms_bit_exact_against_numpy(nms_type, thr, sigma, cap):
    from mtl_ssl_amd import ops
    rng = np.random.RandomState(int(thr * 10) + cap + len(nms_type))
    sizes = [0, 1, 2, 17, 0, 300, 64, ops.EVAL_NMS_MAX_SEGMENT]
    segs = [_segment(rng, n) for n in sizes]
    boxes = np.concatenate([s[0] for s in segs])
    scores = np.concatenate([s[1] for s in segs])
    for scale in ((1.0, 1.0), (480.0, 640.0)):
        idx, sco, cnt = ops.eval_nms(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), sizes,
                                     nms_type, thr, sigma, cap, scale=scale)
        idx, sco, cnt = idx.cpu().numpy(), sco.cpu().numpy(), cnt.cpu().numpy()
        off = 0
        for j, (n, (b, s)) in enumerate(zip(sizes, segs)):
            want_i, want_s = eval_nms_numpy(b, s, np.asarray([scale[0], scale[1]] * 2), nms_type, thr, sigma, cap,
                                            exp=portable_exp)
            m = len(want_i)
            got_i, got_s = idx[off:off + n], sco[off:off + n]
            assert int(cnt[j]) == m, (nms_type, thr, cap, n, scale)
            assert np.array_equal(got_i[:m], want_i), (nms_type, thr, cap, n, scale)
            assert np.array_equal(got_s[:m], want_s), (nms_type, thr, cap, n, scale)
            assert np.all(got_i[m:] == -1)
            off += n


def test_eval_nms_segment_bound_is_a_clean_error():
    from mtl_ssl_amd import lib, ops
    n = ops.EVAL_NMS_MAX_SEGMENT + 1
    b, s = _segment(np.random.RandomState(1), n)
    with pytest.raises(lib.MtlsslError, match="max_total_detections"):
        ops.eval_nms(torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV), [n],
                     "standard", 0.5, 0.5, 100)
    torch.cuda.synchronize()
    # the library is usable afterwards
    idx, sco, cnt = ops.eval_nms(torch.from_numpy(b[:5]).to(DEV), torch.from_numpy(s[:5]).to(DEV), [5],
                                 "standard", 0.5, 0.5, 100)
    assert int(cnt.cpu()[0]) == len(eval_nms_numpy(b[:5], s[:5], 1.0, "standard", 0.5, 0.5, 100)[0])


@pytest.mark.parametrize("Hf,Wf,h,w", [(7, 9, 20, 31), (40, 50, 13, 17), (5, 5, 5, 5), (1, 1, 3, 4), (6, 4, 1, 1),
                                        (38, 50, 150, 200), (13, 7, 9, 29)])
def test_edgemask_agreement_counts_match_numpy(Hf, Wf, h, w):
    from mtl_ssl_amd import ops
    rng = np.random.RandomState(Hf * 100 + w)
    logits = rng.normal(0, 1, (Hf, Wf, 2)).astype(np.float32)
    logits[::2, ::3, 1] = logits[::2, ::3, 0]                   # exact ties: label 0 on both sides
    gt = (rng.uniform(0, 1, (h, w)) < 0.5).astype(np.float32)
    got = ops.edgemask_agreement(torch.from_numpy(logits).to(DEV), torch.from_numpy(gt).to(DEV))
    want = int(np.sum(edgemask_labels_numpy(logits, h, w) == gt))
    assert int(got.cpu()[0]) == want
    # against its own labels the agreement is total
    got = ops.edgemask_agreement(torch.from_numpy(logits).to(DEV),
                                 torch.from_numpy(edgemask_labels_numpy(logits, h, w)).to(DEV))
    assert int(got.cpu()[0]) == h * w
