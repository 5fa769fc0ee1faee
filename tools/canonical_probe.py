#!/usr/bin/env python3
"""What does canonicalising a labelled batch cost?  labelling.canonicalize_flat (one workgroup per graph, nothing read back)
against the per-graph labelling.canonicalize_positive_edges looped over the same graphs, on a 32-graph CWQ-shaped batch
(3 000 nodes / 10 000 edges per graph) and on a 2 000-graph chunk of the same graphs.  Every graph holds 40 groups of three
parallel positive edges, 60 single positives and 4 pair lists of 40 ids; relation table 5 000 x 768.

canonicalize_flat is timed with events on the launch stream (median of --rounds >= 7 samples of --calls calls each; the flat
inputs are on the device, as label_pairs_flat leaves them).  The per-graph loop is host-bound (a dict over the edges, a GEMV
over the whole table and a read-back per graph), so it is timed by the host clock around a loop that ends synchronised (median of
--old-rounds).  GPU only.

  python tools/canonical_probe.py --json-out probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS, GROUP_SIZE, SINGLES, PAIRS, PAIR_IDS = 40, 3, 60, 4, 40


def make_graphs(B, nodes, edges, R, seed):
    """Flat host arrays of B graphs (node ids graph-local in src / dst)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, nodes, (B, edges))
    dst = rng.integers(0, nodes, (B, edges))
    rel = rng.integers(0, R, (B, edges))
    mask = np.zeros((B, edges), bool)
    n_par = GROUPS * GROUP_SIZE
    u, v = rng.integers(0, nodes, (B, GROUPS)), rng.integers(0, nodes, (B, GROUPS))
    flip = rng.random((B, n_par)) < 0.5
    uu, vv = np.repeat(u, GROUP_SIZE, axis=1), np.repeat(v, GROUP_SIZE, axis=1)
    pos = np.stack([rng.permutation(edges)[: n_par + SINGLES] for _ in range(B)])      # where the positives sit
    rows = np.arange(B)[:, None]
    src[rows, pos[:, :n_par]] = np.where(flip, vv, uu)
    dst[rows, pos[:, :n_par]] = np.where(flip, uu, vv)
    mask[rows, pos] = True
    pair_ids = np.stack([np.stack([rng.permutation(pos[b])[:PAIR_IDS] for _ in range(PAIRS)]) for b in range(B)])  # [B, PAIRS, ids]
    return src.astype(np.int64), dst.astype(np.int64), rel.astype(np.int64), mask, pair_ids.astype(np.int64)


def measure_case(name, B, args, dev, qn_all, rn):
    import torch

    from evi_rag_amd import labelling as L

    src, dst, rel, mask, pair_ids = make_graphs(B, args.nodes, args.edges, rn.size(0), seed=B)
    E_g = args.edges
    edge_ptr = np.arange(B + 1, dtype=np.int64) * E_g
    node_off = (np.arange(B, dtype=np.int64) * args.nodes)[:, None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ei = t(np.stack([(src + node_off).reshape(-1), (dst + node_off).reshape(-1)]))
    P = B * PAIRS
    z = np.zeros(P, np.int64)
    flat = L.FlatPairLabels(B, B * E_g, edge_ptr, t(mask.reshape(-1).astype(np.uint8)), torch.ones(P, dtype=torch.int32, device=dev),
                            torch.full((P,), PAIR_IDS, dtype=torch.int32, device=dev),
                            torch.arange(P + 1, dtype=torch.int64, device=dev) * PAIR_IDS,
                            t((pair_ids + edge_ptr[:-1, None, None]).reshape(-1)), np.repeat(np.arange(B, dtype=np.int64), PAIRS), z, z.copy(),
                            np.arange(B + 1, dtype=np.int64) * PAIRS, edge_ptr=t(edge_ptr))
    rel_d, qn = t(rel.reshape(-1)), qn_all[:B].contiguous()

    def new():
        return L.canonicalize_flat(flat, ei, rel_d, qn, rn)

    def old():
        out = []
        for g in range(B):
            out.append(L.canonicalize_positive_edges(src[g], dst[g], rel[g], mask[g], pair_ids[g].reshape(-1).tolist(),
                                                     [PAIR_IDS] * PAIRS, qn[g], rn))
        torch.cuda.synchronize(dev)
        return out

    for _ in range(2):
        res = new()
    torch.cuda.synchronize(dev)
    res.check_deferred()
    new_ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            new()
        e1.record()
        torch.cuda.synchronize(dev)
        new_ms.append(e0.elapsed_time(e1) / args.calls)
    ref = old()  # warm-up of the loop, and the comparison of the results
    keep = res.mask[: flat.E].cpu().numpy().astype(bool).reshape(B, E_g)
    same = all(np.array_equal(keep[g], np.asarray(ref[g][0], bool)) for g in range(B))
    ids_new = res.pair_edge_ids[: int(res.pair_edge_off[-1].item())].cpu().numpy()
    same = same and np.array_equal(ids_new, np.concatenate([np.asarray(ref[g][1], np.int64) + edge_ptr[g] for g in range(B)]))
    old_ms = []
    for _ in range(args.old_rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        old()
        old_ms.append((time.perf_counter() - t0) * 1e3)
    return {"name": name, "graphs": B, "edges": B * E_g, "positives": int(mask.sum()), "new_ms": new_ms, "old_ms": old_ms,
            "same_result": bool(same)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=3000)
    ap.add_argument("--edges", type=int, default=10000)
    ap.add_argument("--relations", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=9, help="event-timed samples of canonicalize_flat (at least 7)")
    ap.add_argument("--calls", type=int, default=5, help="calls per sample")
    ap.add_argument("--old-rounds", type=int, default=3, help="host-timed passes of the per-graph loop")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    import torch

    from evi_rag_amd import ops

    if not torch.cuda.is_available():
        sys.exit("canonical_probe needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = ops.normalize_embeddings(torch.randn(args.relations, args.dim, device=dev, generator=g), 1e-6)
    qn = ops.normalize_embeddings(torch.randn(max(args.batch, args.chunk), args.dim, device=dev, generator=g), 1e-6)
    cases = [measure_case(f"{B}-graph {kind}", B, args, dev, qn, rn) for kind, B in (("batch", args.batch), ("chunk", args.chunk))]
    res = {"device": torch.cuda.get_device_name(dev), "graph": {"nodes": args.nodes, "edges": args.edges}, "relations": args.relations,
           "dim": args.dim, "rounds": args.rounds, "calls_per_round": args.calls, "old_rounds": args.old_rounds, "cases": cases}
    if args.json_out:
        with open(args.json_out, "w", encoding="utf-8") as fh:
            json.dump(res, fh, indent=1)
    for c in cases:
        n, o = c["new_ms"], c["old_ms"]
        print(f"{c['name']}: {c['edges']} edges, {c['positives']} positives; canonicalize_flat {statistics.median(n):.3f} ms "
              f"(min {min(n):.3f}, max {max(n):.3f}); per-graph loop {statistics.median(o):.1f} ms (min {min(o):.1f}, max {max(o):.1f}); "
              f"same result: {'yes' if c['same_result'] else 'NO'}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
