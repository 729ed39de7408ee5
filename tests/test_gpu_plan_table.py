"""Every (problem, mode) of the committed plan table (mtl_ssl_amd/conv_plans.json: the 150 distinct convolution layers of
the four shipped configurations) at its full production size, on the plan production picks — the pinned code where the
table pins one, the library's planner (split-K main + tail + fold, the LDS-DMA engine, the Winograd variants, the padded
/ VALU forms) where it says -1 — against float64.

Every element of every output is compared: tests/conv_ref.py builds the float64 reference of the whole output by a plain
tap walk on the device (ConvCase.check_whole) — a wrong tile in the middle of the grid, a K-step dropped in one dw tile
column, a tile the swizzle maps twice have nowhere to hide — and a miss names row, column, tile and split. Before it the
sampled reference built on the CPU runs as it always did: ~256 flat output rows of the forward (all K channels each)
and input rows of the dgrad (all C channels), tile boundaries and image corners included, and every (r, s) tap of a
16 x 16 channel block of the filter gradient summed over all N*OH*OW pixels. It is the independent check of the device's
float64 reference (held equal to it on the sample to n * 2^-52 * scale) and keeps the report's series of sampled numbers.
Neither shortens a reduction. Errors are measured in units of 2^-24 * (sum |a*b| + |the epilogue's addends|)
(tests/parity_report.py dot_err): at most 8 for a direct plan, 400 for a Winograd plan, on the sample and on the whole
output alike. The nonlinear epilogues (ReLU, the ReLU mask) must be exact functions of the linear result, bit for bit.
The same list then runs through the production Winograd filter cache (ops.FilterXfCache) and the kept input transform,
and on the split-bf16 fp32 engine. Only the modes the table lists for a problem run: those are the calls the model
makes. Workspaces stay NaN-poisoned (conftest: MTLSSL_POISON_WS)."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest
import torch

from tests import parity_report
from tests.conv_ref import DIRECT_BOUND, MODE_NAMES, WINO_BOUND, ConvCase, pid as _pid, plan_test_ops, whole_line

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    plans = json.load(open(os.path.join(ROOT, "mtl_ssl_amd", "conv_plans.json")))["plans"]
    probs = {}
    for key, val in plans.items():
        v = tuple(int(t) for t in key.split(","))
        probs.setdefault(v[1:], {})[v[0]] = val
    return sorted(probs.items())


PROBLEMS = _load()              # [(N, H, W, C, K, R, S, OH, OW, stride, dilation, pad_t, pad_l), {mode: table value}]
_RUN = {}                       # (problem, mode) -> {"cfg", "family", "err", "split", "whole", "whole_split", "elements", "ref_diff"}


@pytest.fixture(scope="module")
def ops():
    yield from plan_test_ops()
    _report()


def _desc(prob):
    from mtl_ssl_amd.lib import ConvDesc
    return ConvDesc(*prob, 0)


def _cfg(d, mode):
    from mtl_ssl_amd.lib import lib
    return lib().conv2d_tile_config(ctypes.byref(d), mode)


def _family(ops, d, mode):
    from mtl_ssl_amd.lib import lib
    return ops.conv_class(_cfg(d, mode), lib().conv2d_executed_macs(ctypes.byref(d), mode, 1))


def _is_wino(ops, cfg):
    return cfg >= 0 and ops.plan_code_algorithm(cfg) in (1, 2)


def _bound(ops, cfg):
    return WINO_BOUND if _is_wino(ops, cfg) else DIRECT_BOUND


def test_parametrization_covers_the_whole_table():
    assert len(PROBLEMS) == 150
    assert sum(len(m) for _, m in PROBLEMS) == 359
    assert len({p for p, _ in PROBLEMS}) == len(PROBLEMS)


@pytest.mark.parametrize("prob,modes", PROBLEMS, ids=[_pid(p) for p, _ in PROBLEMS])
def test_production_plan_matches_float64(ops, prob, modes):
    d = _desc(prob)
    case = ConvCase(prob)
    for mode in sorted(modes):
        case.prepare(mode)
    call = lambda mode, **kw: case.call(ops, d, mode, **kw)
    out = {}                    # mode -> native outputs, reused by the split-engine pass

    for mode, pinned in sorted(modes.items()):
        o = out[mode] = call(mode)
        cfg = _cfg(d, mode)
        # (a) the table takes effect: the first call of the mode applied the pinned code
        if pinned >= 0:
            assert cfg == pinned, ("plan table entry not applied", mode, pinned, cfg)
        case.check_finite(o, mode, cfg)

        def note(errs, lims):
            _RUN[(prob, mode)] = dict(cfg=cfg, family=_family(ops, d, mode), err=errs[0], split=None)
        case.check_errors(mode, o, _bound(ops, cfg), cfg, note)

        def note_whole(errs, lims):
            print("%s: every element %s of %s (sample %.2f)" % (_pid(prob, mode), ["%.2f" % e for e in errs], lims, _RUN[(prob, mode)]["err"]))
            _RUN[(prob, mode)].update(whole=errs[0], whole_split=None, **case.whole_stats[mode])
        case.check_whole(mode, o, _bound(ops, cfg), (MODE_NAMES[mode], cfg), note_whole)

    for mode in (0, 1):
        if mode in modes:
            case.check_exact_epilogue(mode, call(mode, nonlinear=True), out[mode], _cfg(d, mode))

    # (c) production Winograd path: the filter cache and the kept input transform change no bit
    for mode in (0, 1):
        if mode in modes and _is_wino(ops, _cfg(d, mode)):
            cache = ops.FilterXfCache()
            assert torch.equal(call(mode, xf_cache=cache), out[mode]), ("filter cache", mode, _cfg(d, mode))
            assert len(cache.entries) == 1
            assert torch.equal(call(mode, xf_cache=cache), out[mode]), ("filter cache, second use", mode)
    if 0 in modes and 2 in modes and ops._shared_input_variant(d) >= 0:
        keep = {}
        assert torch.equal(call(0, keep_input_xf=keep), out[0])
        dw, db = call(2, input_xf=keep[case.x.data_ptr()])
        assert torch.equal(dw, out[2][0]) and torch.equal(db, out[2][1]), "kept input transform"

    # (d) the split-bf16 engine on the same calls: native bits where it declines, the native accuracy where it engages
    assert ops.set_fp32_engine(1) == 0
    try:
        for mode in sorted(modes):
            o = call(mode)
            same = torch.equal(o[0], out[mode][0]) if mode == 2 else torch.equal(o, out[mode])
            if same:
                continue
            assert not _split_declines(ops, prob, mode, _cfg(d, mode)), ("split engine ran on a small problem", mode)
            e = case.errors(mode, o)[0]
            rec = _RUN[(prob, mode)]
            rec["split"] = e
            assert e <= 1.25 * max(rec["err"], 1.0) + 2.5, (MODE_NAMES[mode], rec, e)
            (e_whole, at), lim = case.whole_errors(mode, o)[0], 1.25 * max(rec["whole"], 1.0) + 2.5
            rec["whole_split"] = e_whole
            assert e_whole <= lim, ("split engine, every element", MODE_NAMES[mode], rec, e_whole, lim, case.describe(mode, 0, at))
    finally:
        ops.set_fp32_engine(0)


def _split_declines(ops, prob, mode, cfg):
    """Problems the split-bf16 engine must leave to the native one (csrc/conv_split.h split_tile_for /
    split_wgrad_plan): a stride-1 direct forward or dgrad with fewer than 192 tiles of 256 x 256 (or an output narrower
    than 256, counted with the GEMM width padded to 16), a filter gradient with C or K below 256."""
    N, H, W, C, K, R, S, OH, OW, stride = prob[:10]
    if mode == 2:
        return C < 256 or K < 256
    rows, cols = (N * OH * OW, K) if mode == 0 else (N * H * W, C)
    cols = -(-cols // 16) * 16
    return stride == 1 and not _is_wino(ops, cfg) and (cols < 256 or -(-rows // 256) * -(-cols // 256) < 192)


def _output_elements(prob, mode):
    """Elements a call of the mode writes: y, dx, or dw and the bias gradient."""
    N, H, W, C, K, R, S, OH, OW = prob[:9]
    return (N * OH * OW * K, N * H * W * C, R * S * C * K + K)[mode]


def _winograd_entries(ops):
    """(problem, mode) of every forward / dgrad the table plans as Winograd."""
    out = []
    for prob, modes in PROBLEMS:
        d = _desc(prob)
        for mode in (0, 1):
            if mode in modes:
                ops._autotune(d, mode, None)          # the plan of the first call (the on-line tuner is off)
                if _is_wino(ops, _cfg(d, mode)):
                    out.append((prob, mode))
    return out


def test_filter_cache_refresh_follows_weight_changes(ops, monkeypatch):
    """All Winograd forward / dgrad entries of the table in ONE cache (both variants, both modes), the weights changed
    in place, refreshed by the batched transform (ops.FilterXfCache.refresh): once on the current stream in the default
    chunks, once on a side stream in many small chunks. After each refresh every cached call gives the uncached bits."""
    entries = _winograd_entries(ops)
    assert len(entries) >= 4
    g = torch.Generator(device="cuda").manual_seed(11)
    weights = {}
    for prob, _ in entries:
        R, S, C, K = prob[5], prob[6], prob[3], prob[4]
        weights.setdefault(prob, torch.empty(R, S, C, K, device="cuda"))

    def new_weights():
        for prob, w in weights.items():
            w.copy_((torch.rand(w.shape, device="cuda", generator=g) - 0.5) * (2.0 / np.sqrt(9 * prob[3])))

    def check_all(cache, tag):
        for prob, mode in entries:
            d, w = _desc(prob), weights[prob]
            gi = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((prob, mode)).encode()))
            shape = (prob[0], prob[1], prob[2], prob[3]) if mode == 0 else (prob[0], prob[7], prob[8], prob[4])
            u = torch.rand(shape, device="cuda", generator=gi) - 0.3
            if mode == 0:
                a, b = ops.conv2d_fwd(d, u, w, xf_cache=cache), ops.conv2d_fwd(d, u, w)
            else:
                a, b = ops.conv2d_dgrad(d, u, w, xf_cache=cache), ops.conv2d_dgrad(d, u, w)
            assert torch.equal(a, b), (tag, _pid(prob), mode, _cfg(d, mode))

    new_weights()
    cache = ops.FilterXfCache()
    check_all(cache, "first use")
    kinds = {(e["variant"], e["mode"]) for e in cache.entries.values()}
    assert len(cache.entries) == len(entries) and {v for v, _ in kinds} == {0, 1} and {m for _, m in kinds} == {0, 1}

    new_weights()
    cache.refresh()
    check_all(cache, "refresh on the current stream")

    new_weights()
    n_default = len(cache._tables())
    monkeypatch.setattr(ops.FilterXfCache, "CHUNK_BYTES", 1 << 20)
    n_chunks = len(cache._tables())
    assert n_chunks > max(n_default, 3), (n_chunks, n_default)
    side = torch.cuda.Stream()
    cache.refresh(stream=side)
    check_all(cache, "refresh on a side stream in %d chunks" % n_chunks)
    torch.cuda.synchronize()
    parity_report.add("plan table, Winograd filter cache: %d forward / dgrad entries (%d variant/mode kinds) equal to "
                      "the uncached calls bit for bit after first use, a refresh on the current stream and one on a side "
                      "stream in %d chunks" % (len(entries), len(kinds), n_chunks))


def _report():
    if not _RUN:
        return
    fams = {}
    for (prob, mode), r in _RUN.items():
        f = fams.setdefault(r["family"], dict(n=0, modes=[0, 0, 0], err=[0.0, 0.0, 0.0], split=[None, None, None], eng=0,
                                              whole=[], whole_split=[None, None, None]))
        f["n"] += 1
        f["modes"][mode] += 1
        f["err"][mode] = max(f["err"][mode], r["err"])
        if r["split"] is not None:
            f["eng"] += 1
            f["split"][mode] = max(f["split"][mode] or 0.0, r["split"])
        if "whole" in r:
            f["whole"].append((mode, r["whole"], r["elements"], r["ref_diff"]))
            if r["whole_split"] is not None:
                f["whole_split"][mode] = max(f["whole_split"][mode] or 0.0, r["whole_split"])
    pinned = sum(1 for prob, m in PROBLEMS for mode, v in m.items() if v >= 0 and (prob, mode) in _RUN)
    parity_report.add("plan table at full size: %d (problem, mode) pairs of %d problems ran (%d pinned, %d on the "
                      "planner's choice); per family (fwd / dgrad / wgrad):" % (
                          len(_RUN), len({p for p, _ in _RUN}), pinned, len(_RUN) - pinned))
    fmt = lambda v: "-" if v is None else "%.2f" % v
    for name, f in sorted(fams.items()):
        parity_report.add("    %-32s %3d pairs (%d / %d / %d); worst error in 2^-24*sum|ab| units native %s, split-bf16 "
                          "%s (engaged on %d)" % (
                              name, f["n"], f["modes"][0], f["modes"][1], f["modes"][2],
                              " / ".join("%.2f" % v for v in f["err"]), " / ".join(fmt(v) for v in f["split"]), f["eng"]))
        if f["whole"]:
            parity_report.add(whole_line(f["whole"]) + "; split-bf16 %s" % " / ".join(fmt(v) for v in f["whole_split"]))
    # coverage: what was compared is every element of every output of the pairs that ran — of all 359 when all ran
    compared = sum(r.get("elements", 0) for r in _RUN.values())
    pairs, table = sum(len(m) for _, m in PROBLEMS), sum(_output_elements(p, m) for p, ms in PROBLEMS for m in ms)
    parity_report.add("    every output element compared with float64: %d elements of %d pairs (the table's %d pairs write %d)" % (
        compared, len(_RUN), pairs, table))
    assert compared == sum(_output_elements(p, m) for p, m in _RUN), "a (problem, mode) pair was not compared whole"
    assert len(_RUN) < pairs or compared == table, (compared, table)     # the whole table ran: every element it writes
    engaged = [key for key, r in _RUN.items() if r["split"] is not None]
    parity_report.add("    split-bf16 engine engaged on %d of %d (problem, mode) pairs (%d problems); native bits on the rest" % (
        len(engaged), len(_RUN), len({p for p, _ in engaged})))
