#!/usr/bin/env python3
"""What does the row filter cost the exact scan?  ops.cosine_topk (method "scan") at 2^23 x 768 f32, Q = 32, k = 500:
unfiltered, an all-true mask, a 50 % mask, a 1 % mask and six labels with mixed allow-sets.  The cases alternate inside
every round; the table holds the median (and min - max) of the rounds' per-call times, plus the per-kernel split of one
extra timed call per case (the library's own launch events: index scan / selections).  GPU only.

  python tools/topk_filter_probe.py --json-out probe.json                 # measure (needs the GPU)
  python tools/topk_filter_probe.py --from-json probe.json --write-design DESIGN.md   # put the table into DESIGN.md
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- topk_filter_probe:begin -->", "<!-- topk_filter_probe:end -->"


def measure(args):
    import torch

    from evi_rag_amd import _lib, ops

    dev = torch.device("cuda:0")
    N, D, Q, k = args.rows, args.dim, args.queries, args.k
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.empty((N, D), dtype=torch.float32, device=dev)
    for a in range(0, N, 1 << 20):  # chunked: no second copy of the index
        ops.normalize_embeddings(torch.randn(min(1 << 20, N - a), D, device=dev, generator=g), out=x[a: a + (1 << 20)])
    q = ops.normalize_embeddings(torch.randn(Q, D, device=dev, generator=g))
    u = torch.rand(N, device=dev, generator=g)
    labels6 = torch.randint(0, 6, (N,), device=dev, generator=g, dtype=torch.int64).to(torch.uint8)
    allow6 = torch.tensor([[0b111111, 0b000111, 0b101010, 0b000001][i % 4] for i in range(Q)], dtype=torch.int32, device=dev)
    cases = [
        ("unfiltered", {}),
        ("all-true mask", {"row_mask": torch.ones(N, dtype=torch.bool, device=dev)}),
        ("50 % mask", {"row_mask": u < 0.5}),
        ("1 % mask", {"row_mask": u < 0.01}),
        ("six labels, mixed allow-sets", {"row_labels": labels6, "query_allow": allow6}),
    ]
    ws = torch.empty(ops.cosine_topk_workspace_bytes(Q, N, D, k), dtype=torch.uint8, device=dev)
    out = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev))

    def call(kw):
        ops.cosine_topk(q, x, k, method="scan", workspace=ws, out=out, **kw)

    for _, kw in cases:  # every instantiation loaded, every shape warm
        for _ in range(2):
            call(kw)
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in cases}
    for _ in range(args.rounds):
        for name, kw in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call(kw)
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1) / args.calls)
    lib = _lib.load()
    split = {}
    for name, kw in cases:  # the per-kernel split, in calls of their own
        lib.evi_timing_enable(1)
        for _ in range(args.calls):
            call(kw)
        torch.cuda.synchronize(dev)
        lib.evi_timing_enable(0)
        ms, launches = (ctypes.c_double * 4)(), (ctypes.c_int32 * 4)()
        _lib.check(lib.evi_timing_read(ms, launches, 4))
        split[name] = {"scan_ms": ms[0] / args.calls, "select_ms": ms[1] / args.calls}
    return {"shape": {"rows": N, "dim": D, "queries": Q, "k": k}, "rounds": args.rounds, "calls_per_round": args.calls,
            "device": torch.cuda.get_device_name(dev),
            "cases": [{"name": name, "ms_per_call": times[name], **split[name]} for name, _ in cases]}


def table(res):
    s = res["shape"]
    base = statistics.median(res["cases"][0]["ms_per_call"])
    lines = [f"Filtered scan cost (`tools/topk_filter_probe.py`, {res['device']}): {s['rows']} x {s['dim']} f32, Q = {s['queries']}, "
             f"k = {s['k']}, method \"scan\"; median of {res['rounds']} alternating rounds of {res['calls_per_round']} calls "
             "(min - max of the rounds), and the kernels' own times from one further timed pass.", "",
             "| case | ms per call (median) | min - max | vs unfiltered | index scan kernels ms | selections ms |",
             "|---|---|---|---|---|---|"]
    for c in res["cases"]:
        t = c["ms_per_call"]
        med = statistics.median(t)
        lines.append(f"| {c['name']} | {med:.3f} | {min(t):.3f} - {max(t):.3f} | {(med / base - 1) * 100:+.2f} % | "
                     f"{c['scan_ms']:.3f} | {c['select_ms']:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1 << 23)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9, help="alternating rounds (at least 7)")
    ap.add_argument("--calls", type=int, default=10, help="calls per case per round")
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
