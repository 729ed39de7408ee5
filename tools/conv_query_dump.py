"""Every host-side answer of the conv planner, one text line per (problem, mode, planner state): for comparing two builds.

    python tools/conv_query_dump.py OUT.txt

Host only (no GPU). Run it in two checkouts and compare the files: a refactor of csrc/conv.hip's plan resolution must leave
them byte-identical. Cases: every problem of tools/offtable_plan_sweep.sweep() and an off-path grid (padded, thin, small-GEMM,
stem, scalar and whole-7-span Winograd problems the sweep does not meet) in all three modes under set_winograd 0 / 1 / 2, and
the plan table's pairs with their table code pinned and with each of the 24 plan codes and -1 forced. The summary counts
plan_info's family per mode, which shows what the cases reach.
"""
import collections
import ctypes
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import offtable_plan_sweep as sweep_tool                                   # noqa: E402

MAPS = ((1, 1), (5, 7), (14, 14), (38, 64))
CHANNELS = (3, 4, 8, 13, 16, 21, 24, 40, 64, 91, 189, 364)


def grid(ops):
    for n, (h, w), c, k, r, st, dil, pad in itertools.product((1, 3), MAPS, CHANNELS, CHANNELS, (1, 3, 7), (1, 2), (1, 2),
                                                              ("SAME", "VALID")):
        if pad == "VALID" and (h < (r - 1) * dil + 1 or w < (r - 1) * dil + 1):
            continue                                                       # no output pixel
        d = ops.conv_desc((n, h, w, c), (r, r, c, k), st, dil, pad)
        yield d
        if k % 4 == 0:
            e = ops.conv_desc((n, h, w, c), (r, r, c, k), st, dil, pad)
            e.ldy = k + 16
            yield e


def answers(L, d, mode):
    ref = ctypes.byref(d)
    out = [L.conv2d_workspace_bytes(ref, mode), L.conv2d_wgrad_workspace_bytes(ref), L.conv2d_tile_config(ref, mode),
           L.conv2d_executed_macs(ref, mode, 1), L.conv2d_executed_macs(ref, mode, 0), L.conv2d_num_dispatches(ref, mode)]
    info = (ctypes.c_int32 * 16)()
    for cls in range(4):
        out.append(L.cdll.mtlssl_conv2d_plan_info(ref, mode, cls, info))   # unchecked: the return code is an answer
        out.extend(info)
    out += [L.conv2d_filter_xf_bytes(ref, mode), L.conv2d_filter_xf_variant(ref, mode), L.conv2d_input_xf_bytes(ref, 0),
            L.conv2d_input_xf_bytes(ref, 1), L.conv2d_wgrad_grouped_workspace_bytes(ref, 1),
            L.conv2d_wgrad_grouped_workspace_bytes(ref, 3)]
    return out, info[0] if out[6] == 0 else -1


def main(path):
    swept = sorted({q[0] for q in sweep_tool.sweep()["queried"]})          # builds the library, leaves the tuning reset
    from mtl_ssl_amd import ops
    from mtl_ssl_amd.lib import lib
    L = lib()
    sha, reached, n = hashlib.sha256(), collections.Counter(), 0
    with open(path, "w") as f:
        def dump(tag, d, mode):
            nonlocal n
            ans, family = answers(L, d, mode)
            line = "%s %d %s | %s\n" % (tag, mode, " ".join(str(getattr(d, k)) for k, _ in d._fields_), " ".join(map(str, ans)))
            f.write(line)
            sha.update(line.encode())
            reached[(mode, ops.PLAN_FAMILIES[family] if family >= 0 else "error")] += 1
            n += 1

        descs = [sweep_tool.desc_of(p) for p in swept] + list(grid(ops))
        for wino in (0, 1, 2):
            ops.reset_tuning(False, False)
            prev = ops.set_winograd(wino)
            for d in descs:
                for mode in (0, 1, 2):
                    dump("wino%d" % wino, d, mode)
            ops.set_winograd(prev)
        ops.reset_tuning(True, False)
        pairs = [(sweep_tool.desc_of(p), m) for p, modes in sorted(sweep_tool.table_problems().items()) for m in modes]
        for d, mode in pairs:
            ops._autotune(d, mode, None)                                   # pins the table's code like a first call does
            dump("table", d, mode)
        ops.reset_tuning(False, False)
        for d, mode in pairs:
            for code in list(range(24)) + [-1]:
                L.conv2d_force_config(ctypes.byref(d), mode, code)
                dump("force%d" % code, d, mode)
    for key, cnt in sorted(reached.items()):
        print("mode %d %-16s %d" % (key[0], key[1], cnt))
    print("%d cases, sha256 %s" % (n, sha.hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1])
