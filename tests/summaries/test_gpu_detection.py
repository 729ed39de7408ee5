"""mtlssl_variable_histograms against the float64 restatement of TensorFlow's Histogram::Add
(summaries.histogram_numpy): bucket counts, min, max and num bit for bit; sum and sum_squares within the worst case of
any double summation order, n * 2^-53 * sum(|term|) around math.fsum — derived, not measured.

Sizes sit on every edge of the kernel: empty, one element, around the 64-float alignment unit, around the chunk length
C (one workgroup per chunk: C-1, C, C+1, and 3C+7 = four chunks with a ragged tail that is no multiple of a 16-byte
load). The alignment padding holds 1e30, which would show in sum / counts if it were ever counted.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by module
name, and these kernel-level tests run in its first stage, ahead of every whole-model case."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, np.float32(1e-12)], np.float32)
PAD = np.float32(1e30)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _layout(sizes):
    offsets, off = [], 0
    for s in sizes:
        offsets.append(off)
        off += -(-s // 64) * 64
    return offsets, off + 64


@pytest.fixture(scope="module")
def case():
    """(host buffer, offsets, sizes, per-variable restatement) — computed once, never written again."""
    from mtl_ssl_amd import ops, summaries
    C = ops.HISTOGRAM_CHUNK
    sizes = [0, 1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]
    offsets, total = _layout(sizes)
    rng = np.random.RandomState(11)
    host = np.full(total, PAD, np.float32)
    for o, s in zip(offsets, sizes):
        host[o:o + s] = (rng.standard_normal(s) * 0.09).astype(np.float32)
    lim = summaries.default_bucket_limits()
    edge = []
    for i in np.linspace(1, len(lim) - 2, 20).astype(int):          # limits a float32 can stand next to
        f = np.float32(lim[i])
        edge += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    extra = np.concatenate([SPECIAL, np.array(edge, np.float32)])
    big = host[offsets[-1]:offsets[-1] + sizes[-1]]
    where = np.concatenate([rng.choice(3 * C, len(extra) - 4, replace=False), 3 * C + np.array([3, 4, 5, 6])])
    big[where] = extra                                               # four of them in the ragged tail of the last chunk
    host.setflags(write=False)
    want = [summaries.histogram_numpy(host[o:o + s]) for o, s in zip(offsets, sizes)]
    return host, offsets, sizes, want


def _check(host, offsets, sizes, moments, counts, want):
    assert moments.shape == (len(sizes), 6) and moments.dtype == np.float64
    assert counts.shape == (len(sizes), len(want[0][1])) and counts.dtype == np.uint32
    for v, (o, s) in enumerate(zip(offsets, sizes)):
        m, c = want[v]
        np.testing.assert_array_equal(counts[v], c, err_msg="variable %d (size %d)" % (v, s))
        assert moments[v, 0] == m[0] and moments[v, 1] == m[1] and moments[v, 2] == m[2] and moments[v, 5] == m[5], (v, s)
        x = host[o:o + s].astype(np.float64)
        x = x[np.isfinite(x)]
        for k, terms in ((3, x), (4, x * x)):
            exact = math.fsum(terms)
            bound = len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms))
            print("variable %d size %d moment %d: |got - fsum| = %.3e, bound %.3e" % (v, s, k, abs(moments[v, k] - exact), bound))
            assert abs(moments[v, k] - exact) <= bound, (v, s, k, moments[v, k], exact, bound)


def test_every_edge_size_matches_the_restatement_and_two_launches_agree(case):
    from mtl_ssl_amd import ops
    host, offsets, sizes, want = case
    buf = torch.from_numpy(np.array(host)).cuda()
    m1, c1 = ops.variable_histograms(buf, offsets, sizes)
    m2, c2 = ops.variable_histograms(buf, offsets, sizes)
    assert (m1 == m2).all() and (c1 == c2).all()
    assert m1[0, 0] == sys.float_info.max and m1[0, 1] == -sys.float_info.max and m1[0, 2] == 0 and not c1[0].any()
    _check(host, offsets, sizes, m1, c1, want)


def test_non_finite_values_are_counted_apart(case, tmp_path):
    from mtl_ssl_amd import ops, summaries
    host, offsets, sizes, want = case
    h = np.array(host)
    v = 6                                                              # the variable of exactly one chunk
    for j, bad in zip((0, 77, sizes[v] - 1), (np.nan, np.inf, -np.inf)):
        h[offsets[v] + j] = bad
    buf = torch.from_numpy(h).cuda()
    moments, counts = ops.variable_histograms(buf, offsets, sizes)
    assert moments[v, 5] == 3 and moments[v, 2] == sizes[v] - 3
    assert (np.delete(moments[:, 5], v) == 0).all()
    want = list(want)
    want[v] = summaries.histogram_numpy(h[offsets[v]:offsets[v] + sizes[v]])
    _check(h, offsets, sizes, moments, counts, want)
    with summaries.SummaryWriter(str(tmp_path)) as w:
        w.add_histogram("fine", moments[v - 1], counts[v - 1], summaries.default_bucket_limits(), 1)
        with pytest.raises(FloatingPointError, match="Nan in summary histogram for: scope/broken"):
            w.add_histogram("scope/broken", moments[v], counts[v], summaries.default_bucket_limits(), 1)


def test_limits_beyond_lds_and_a_small_workspace_are_refused(case):
    from mtl_ssl_amd import ops
    from mtl_ssl_amd.lib import MtlsslError, lib, ptr
    host, offsets, sizes, _ = case
    buf = torch.from_numpy(np.array(host)).cuda()
    too_many = np.arange(ops.HISTOGRAM_MAX_LIMITS + 1, dtype=np.float64)
    with pytest.raises(MtlsslError, match=r"%d bucket limits, the limit table and the counts of one workgroup hold at "
                                          r"most %d in LDS" % (len(too_many), ops.HISTOGRAM_MAX_LIMITS)):
        ops.variable_histograms(buf, offsets, sizes, limits=too_many)
    m, c = ops.variable_histograms(buf, offsets, sizes, limits=too_many[:-1])      # the largest table that fits
    assert c.shape == (len(sizes), ops.HISTOGRAM_MAX_LIMITS) and int(c.sum()) == int(m[:, 2].sum()) == sum(sizes)
    t = ops.HistogramTables(offsets, sizes, buf.device)
    need = int(lib().variable_histograms_workspace_bytes(t.num_chunks))
    assert need == t.num_chunks * 6 * 8 and t.num_chunks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 4
    lim = torch.from_numpy(too_many[:8].copy()).cuda()
    moments = torch.empty((len(sizes), 6), dtype=torch.float64, device="cuda")
    counts = torch.empty((len(sizes), 8), dtype=torch.int32, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(MtlsslError, match=r"workspace of %d bytes, %d chunks need %d" % (need - 1, t.num_chunks, need)):
        lib().variable_histograms(ptr(buf), ptr(t.offsets), ptr(t.sizes), len(sizes), ptr(t.chunk_table), t.num_chunks,
                                  ptr(lim), 8, ptr(moments), ptr(counts), ptr(ws), need - 1,
                                  torch.cuda.current_stream().cuda_stream)


def test_param_store_histograms_of_the_smoke_mobilenet_model():
    from mtl_ssl_amd import config, model_builder, summaries
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "smoke_mobilenet_v1_mtl.config")).read())
    ps = model_builder.build(cfg.model, True, "cuda", seed=4).ps
    got = ps.histograms()
    assert list(got) == [s.name for s in ps.specs] and any(not s.trainable for s in ps.specs)
    assert ps.histograms() is not got and set(ps._hist_tables) == {0, 1}           # the chunk tables are kept
    host = {True: ps.weights.cpu().numpy(), False: ps.frozen.cpu().numpy()}
    for s in ps.specs:
        x = host[s.trainable][s.offset:s.offset + s.size]
        m, c = summaries.histogram_numpy(x)
        gm, gc = got[s.name]
        np.testing.assert_array_equal(gc, c, err_msg=s.name)
        assert gm[0] == m[0] and gm[1] == m[1] and gm[2] == m[2] == s.size and gm[5] == 0, s.name
        x64 = x.astype(np.float64)
        for k, terms in ((3, x64), (4, x64 * x64)):
            assert abs(gm[k] - math.fsum(terms)) <= len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms)), (s.name, k)
