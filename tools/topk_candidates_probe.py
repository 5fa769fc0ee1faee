#!/usr/bin/env python3
"""What does a top-k over per-query candidate lists cost?  ops.cosine_topk_candidates against the way to get the same
result without it — per query, `index[ids]` into a second index and `ops.cosine_topk(..., method="scan")` over that — at
2^23 x 768, Q = 32, k = 500, f32 and f16 tables: lists of 1 536, 4 096 and 65 536 random distinct ids, and one
relation-shaped case (4 096 entries drawn from 300 ids).  The two versions alternate inside every round; the table holds
the median (and min - max) of the rounds' per-call device-event times, the scoring and selection kernels' own times
from one further timed pass (the library's launch events), and the scoring kernel's rate in distinct rows x row bytes.
The comparator is handed the DISTINCT ids of every list (it has no de-duplication of its own).  GPU only.

  python tools/topk_candidates_probe.py --json-out probe.json                 # measure (needs the GPU)
  python tools/topk_candidates_probe.py --from-json probe.json --write-design DESIGN.md   # put the table into DESIGN.md
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \\
      python tools/topk_candidates_probe.py --profile-case "4096 distinct" --dtype f32        # launches of one case, untimed
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- topk_candidates_probe:begin -->", "<!-- topk_candidates_probe:end -->"
CASES = (("1536 distinct", 1536, None), ("4096 distinct", 4096, None), ("65536 distinct", 65536, None),
         ("4096 entries, 300 distinct", 4096, 300))


def build_table(args, dtype):
    import torch

    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    N, D = args.rows, args.dim
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.empty((N, D), dtype=torch.float16 if dtype == "f16" else torch.float32, device=dev)
    for a in range(0, N, 1 << 20):  # chunked: no second copy of the index
        x[a: a + (1 << 20)] = ops.normalize_embeddings(torch.randn(min(1 << 20, N - a), D, device=dev, generator=g))
    q = ops.normalize_embeddings(torch.randn(args.queries, D, device=dev, generator=g))
    return dev, q, x


def build_lists(args, dev, length, distinct):
    """(cand_ids [Q * length], cand_ptr, per-query distinct ids) of one case."""
    import torch

    g = torch.Generator(device=dev).manual_seed(length + (distinct or 0))
    lists, uniq = [], []
    for _ in range(args.queries):
        if distinct is None:
            L = torch.randint(0, args.rows, (length + length // 8,), device=dev, generator=g).unique()
            L = L[torch.randperm(L.numel(), device=dev, generator=g)][:length]  # distinct, in random order
        else:
            pool = torch.randint(0, args.rows, (distinct,), device=dev, generator=g)
            L = pool[torch.randint(0, distinct, (length,), device=dev, generator=g)]
        lists.append(L)
        uniq.append(L.unique())
    ptr = torch.arange(args.queries + 1, dtype=torch.int64, device=dev) * length
    return torch.cat(lists), ptr, uniq


def measure_dtype(args, dtype):
    import torch

    from evi_rag_amd import _lib, ops

    dev, q, x = build_table(args, dtype)
    Q, k = args.queries, args.k
    lib = _lib.load()
    out = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev))
    ref = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev))
    rows = []
    for name, length, distinct in CASES:
        ids, ptr, uniq = build_lists(args, dev, length, distinct)
        ws = torch.empty(int(lib.evi_cosine_topk_candidates_workspace_bytes(Q, ids.numel(), k)), dtype=torch.uint8, device=dev)

        def new():
            ops.cosine_topk_candidates(q, x, ids, k, cand_ptr=ptr, workspace=ws, out=out)

        def old():
            for i in range(Q):
                ops.cosine_topk(q[i:i + 1], x[uniq[i]], k, method="scan", out=(ref[0][i:i + 1], ref[1][i:i + 1]))

        for _ in range(2):
            new()
            old()
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)))
        local = torch.stack([torch.where(ref[1][i] >= 0, uniq[i][ref[1][i].clamp(min=0)], ref[1][i]) for i in range(Q)])
        same = same and bool(torch.equal(out[1], local))
        times = {"new": [], "old": []}
        for _ in range(args.rounds):
            for tag, fn in (("new", new), ("old", old)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                times[tag].append(e0.elapsed_time(e1) / args.calls)
        lib.evi_timing_enable(1)
        for _ in range(args.calls):
            new()
        torch.cuda.synchronize(dev)
        lib.evi_timing_enable(0)
        ms, launches = (ctypes.c_double * 4)(), (ctypes.c_int32 * 4)()
        _lib.check(lib.evi_timing_read(ms, launches, 4))
        n_distinct = sum(int(u.numel()) for u in uniq)
        rows.append({"name": name, "dtype": dtype, "entries": int(ids.numel()), "distinct_rows": n_distinct,
                     "row_bytes": x.shape[1] * x.element_size(), "same_bits": same, "new_ms": times["new"], "old_ms": times["old"],
                     "score_ms": ms[0] / args.calls, "select_ms": ms[1] / args.calls})
    return rows, torch.cuda.get_device_name(dev)


def measure(args):
    cases, device = [], None
    for dtype in args.dtypes:
        rows, device = measure_dtype(args, dtype)
        cases += rows
        import torch

        from evi_rag_amd import ops

        ops.release_workspaces()
        torch.cuda.empty_cache()
    return {"shape": {"rows": args.rows, "dim": args.dim, "queries": args.queries, "k": args.k}, "rounds": args.rounds,
            "calls_per_round": args.calls, "device": device, "cases": cases}


def profile_case(args):
    """The launches of one case, untimed, for a kernel trace taken from outside."""
    import torch

    from evi_rag_amd import ops

    name, length, distinct = next(c for c in CASES if c[0] == args.profile_case)
    dev, q, x = build_table(args, args.dtypes[0])
    ids, ptr, _ = build_lists(args, dev, length, distinct)
    for _ in range(args.calls * 4):
        ops.cosine_topk_candidates(q, x, ids, args.k, cand_ptr=ptr)
    torch.cuda.synchronize(dev)
    print(f"profiled {args.calls * 4} calls of '{name}' on the {args.dtypes[0]} table", flush=True)


def table(res):
    s = res["shape"]
    lines = [f"Candidate-list top-k (`tools/topk_candidates_probe.py`, {res['device']}): table {s['rows']} x {s['dim']}, Q = {s['queries']}, "
             f"k = {s['k']}; `cosine_topk_candidates` against per-query `index[ids]` + `cosine_topk(method=\"scan\")` on the distinct ids; "
             f"median of {res['rounds']} alternating rounds of {res['calls_per_round']} calls (min - max of the rounds); scoring and "
             "selection kernel times from one further timed pass; rate = distinct rows x row bytes / scoring kernel time.", "",
             "| table | lists (per query) | new ms (median) | min - max | gather + scan ms (median) | min - max | speed-up | "
             "scoring ms | selection ms | scoring TB/s | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        n, o = c["new_ms"], c["old_ms"]
        rate = c["distinct_rows"] * c["row_bytes"] / (c["score_ms"] * 1e-3) / 1e12 if c["score_ms"] > 0 else float("nan")
        lines.append(f"| {c['dtype']} | {c['name']} | {statistics.median(n):.3f} | {min(n):.3f} - {max(n):.3f} | "
                     f"{statistics.median(o):.3f} | {min(o):.3f} - {max(o):.3f} | {statistics.median(o) / statistics.median(n):.1f} x | "
                     f"{c['score_ms']:.4f} | {c['select_ms']:.4f} | {rate:.2f} | {'yes' if c['same_bits'] else 'NO'} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1 << 23)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f16"], choices=["f32", "f16"])
    ap.add_argument("--rounds", type=int, default=9, help="alternating rounds (at least 7)")
    ap.add_argument("--calls", type=int, default=5, help="calls per version per round")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--from-json", default=None, help="format an earlier measurement instead of measuring")
    ap.add_argument("--profile-case", default=None, choices=[c[0] for c in CASES],
                    help="run only the new call of this case on the first --dtypes table (for a kernel trace)")
    ap.add_argument("--write-design", metavar="DESIGN.md", default=None,
                    help=f"replace the text between the {BEGIN} / {END} markers of this file with the table")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    if args.profile_case:
        return profile_case(args)
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
