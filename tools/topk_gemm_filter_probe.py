#!/usr/bin/env python3
"""What does the row filter cost the GEMM-shaped many-query pass, and how far does the filtered pass beat the filtered
scan?  The config-4 shard (12.5 M x 768 f16) at Q = 512, k = 500, with an all-visible, a 50 % and a 1 % mask (labels
drawn independently per row).  Per mask, alternating inside every round:
  (a) ops.cosine_topk_gemm, unfiltered            (b) ops.cosine_topk_gemm(row_mask=...)
  (c) ops.cosine_topk(row_mask=..., method="scan")  — 16 passes over the index
Each figure is the median (min - max) of the rounds' host-timed calls, read-back of the proof flag included.

--parent-lib PATH: a libevi_hip.so built from the parent commit.  The unfiltered pass is then also timed through the C
ABI (evi_cosine_topk_gemm_f16, device events, one selection precision) for both builds, alternating: the branch must sit
inside the parent's own run-to-run spread.  GPU only.

  python tools/topk_gemm_filter_probe.py --json-out probe.json [--parent-lib parent/libevi_hip.so]
  python tools/topk_gemm_filter_probe.py --from-json probe.json --write-design DESIGN.md
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- topk_gemm_filter_probe:begin -->", "<!-- topk_gemm_filter_probe:end -->"


def _index(N, D, dev, g):
    import torch

    from evi_rag_amd import ops

    x = torch.empty((N, D), dtype=torch.float16, device=dev)
    for a in range(0, N, 1 << 20):  # chunked: the f32 rows never exist as a whole
        x[a: a + (1 << 20)] = ops.normalize_embeddings(torch.randn(min(1 << 20, N - a), D, device=dev, generator=g)).half()
    return x


def _ab_unfiltered(args, q, x, k, products, dev):
    """(a) through the C ABI of the parent and of this build, alternating; ms per call by device events."""
    import torch

    from evi_rag_amd import _lib

    branch = _lib.load()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    Q, D = q.shape
    N = x.size(0)
    sig_ws, sig = _lib.bound_symbols()["evi_cosine_topk_gemm_workspace_bytes"], _lib.bound_symbols()["evi_cosine_topk_gemm_f16"]
    parent.evi_cosine_topk_gemm_workspace_bytes.restype, parent.evi_cosine_topk_gemm_workspace_bytes.argtypes = sig_ws
    parent.evi_cosine_topk_gemm_f16.restype, parent.evi_cosine_topk_gemm_f16.argtypes = sig
    need = max(int(lib.evi_cosine_topk_gemm_workspace_bytes(Q, N, D, k)) for lib in (branch, parent))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_s = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    builds = (("parent", parent), ("branch", branch))

    def call(lib):
        rc = lib.evi_cosine_topk_gemm_f16(q.data_ptr(), Q, x.data_ptr(), N, D, None, k, 0, products, out_s.data_ptr(), out_i.data_ptr(),
                                          status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            sys.exit(f"evi_cosine_topk_gemm_f16 returned {rc}")

    results = {}
    for name, lib in builds:
        call(lib)
        call(lib)
        torch.cuda.synchronize(dev)
        results[name] = (out_s.clone(), out_i.clone(), int(status.item()))
    same = (torch.equal(results["parent"][1], results["branch"][1])
            and torch.equal(results["parent"][0].view(torch.int32), results["branch"][0].view(torch.int32)))
    times = {name: [] for name, _ in builds}
    for _ in range(args.rounds):
        for name, lib in builds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(lib)
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1))
    return {"products": products, "status": {n: results[n][2] for n in results}, "same_result": bool(same), "ms_per_call": times}


def measure(args):
    import torch

    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    N, D, Q, k = args.rows, args.dim, args.queries, args.k
    g = torch.Generator(device=dev).manual_seed(1)
    x = _index(N, D, dev, g)
    q = ops.normalize_embeddings(torch.randn(Q, D, device=dev, generator=g))
    u = torch.rand(N, device=dev, generator=g)
    masks = [("all visible", torch.ones(N, dtype=torch.bool, device=dev)), ("50 % visible", u < 0.5), ("1 % visible", u < 0.01)]
    del u
    out = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev))
    ws = torch.empty(ops.cosine_topk_workspace_bytes(Q, N, D, k), dtype=torch.uint8, device=dev)

    def gemm(m):
        ops.cosine_topk_gemm(q, x, k, out=out, **({} if m is None else {"row_mask": m}))  # `products` 0 in the table: the scan ran

    def scan(m):
        ops.cosine_topk(q, x, k, method="scan", workspace=ws, out=out, row_mask=m)

    def timed(fn, m):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(m)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    cases = []
    for name, m in masks:
        want = ops.cosine_topk(q, x, k, method="scan", row_mask=m)  # also the warm-up of (c)
        gemm(None)
        unfiltered_products = ops.cosine_topk_gemm.last_products
        gemm(m)
        gemm(m)
        products = ops.cosine_topk_gemm.last_products
        same = torch.equal(out[1], want[1]) and torch.equal(out[0].view(torch.int32), want[0].view(torch.int32))
        t = {"a": [], "b": [], "c": []}
        for _ in range(args.rounds):
            t["a"].append(timed(gemm, None))
            t["b"].append(timed(gemm, m))
            t["c"].append(timed(scan, m))
        cases.append({"name": name, "visible_rows": int(m.sum().item()), "products": products, "unfiltered_products": unfiltered_products,
                      "equals_filtered_scan": bool(same), "gemm_ms": t["a"], "gemm_filtered_ms": t["b"], "scan_filtered_ms": t["c"]})
    res = {"shape": {"rows": N, "dim": D, "queries": Q, "k": k}, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev),
           "cases": cases}
    if args.parent_lib:
        res["unfiltered_ab"] = _ab_unfiltered(args, q, x, k, int(cases[0]["unfiltered_products"] or 3), dev)
    return res


def _mmm(t):
    return f"{statistics.median(t):.2f} ({min(t):.2f} - {max(t):.2f})"


def table(res):
    s = res["shape"]
    lines = [f"Filtered many-query pass (`tools/topk_gemm_filter_probe.py`, {res['device']}): {s['rows']} x {s['dim']} f16, "
             f"Q = {s['queries']}, k = {s['k']}; ms per call, median (min - max) of {res['rounds']} alternating rounds, host-timed "
             "with the read-back of the proof flag.", "",
             "| mask | visible rows | (a) GEMM pass, unfiltered | (b) GEMM pass, filtered | (c) scan, filtered (16 passes) | (b) vs (a) | (c) / (b) | "
             "products | (b) == (c) bit for bit |",
             "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        a, b, sc = (statistics.median(c[key]) for key in ("gemm_ms", "gemm_filtered_ms", "scan_filtered_ms"))
        lines.append(f"| {c['name']} | {c['visible_rows']} | {_mmm(c['gemm_ms'])} | {_mmm(c['gemm_filtered_ms'])} | "
                     f"{_mmm(c['scan_filtered_ms'])} | {(b / a - 1) * 100:+.1f} % | {sc / b:.2f}x | {c['products']} | "
                     f"{'yes' if c['equals_filtered_scan'] else 'NO'} |")
    ab = res.get("unfiltered_ab")
    if ab:
        p, b = ab["ms_per_call"]["parent"], ab["ms_per_call"]["branch"]
        lines += ["", f"Unfiltered pass, parent build against this one (C ABI, products = {ab['products']}, device events, alternating calls): "
                      f"parent {_mmm(p)} ms, this build {_mmm(b)} ms; same ids and score bits: {'yes' if ab['same_result'] else 'NO'}."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9, help="alternating rounds (at least 7)")
    ap.add_argument("--parent-lib", default=None, help="libevi_hip.so of the parent commit for the unfiltered A/B")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--from-json", default=None, help="format an earlier measurement instead of measuring")
    ap.add_argument("--write-design", metavar="DESIGN.md", default=None,
                    help=f"replace the text between the {BEGIN} / {END} markers of this file with the table")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    if args.from_json:
        with open(args.from_json, "r", encoding="utf-8") as fh:
            res = json.load(fh)
    else:
        res = measure(args)
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as fh:
            json.dump(res, fh, indent=1)
    text = table(res)
    print(text, flush=True)
    if args.write_design:
        with open(args.write_design, "r", encoding="utf-8") as fh:
            doc = fh.read()
        a, b = doc.find(BEGIN), doc.find(END)
        if a < 0 or b < a:
            sys.exit(f"{args.write_design}: markers {BEGIN} ... {END} not found")
        with open(args.write_design, "w", encoding="utf-8") as fh:
            fh.write(doc[: a + len(BEGIN)] + "\n" + text + "\n" + doc[b:])


if __name__ == "__main__":
    main()
