"""MXFP8 encoder linears (evi_rag_amd.mx) against the bf16 / f32 paths on one MI355X.

  python tools/mx_encode_bench.py [--out FILE] [--skip-linear] [--skip-encode] [--trace-only]

* linear: mx_linear (bf16 in, bf16 out, bias) against F.linear on bf16 operands (hipBLASLt, what bf16 autocast runs once
  the weight is cast) at M in {2048, 8192, 32768} and the bge / BERT (K, N) shapes; device events, every variant warmed,
  the variants alternated within each repetition, median of the repetitions.  TFLOP/s and the share of the 5 PF dense fp8
  and 2.5 PF dense bf16 peaks.
* encode: the bench.py config-5 workload (random-init BERT 24L/1024H, 4 096 texts of 8..32 tokens) at batches of 64 and
  512 with graph replay on, texts/s of f32, bf16 autocast, mxfp8 and mxfp8 + bf16 autocast (alternated, best of the
  repetitions), and overlap@100 / max relative row error of each table against the f32 table.
* --trace-only: two passes of the mxfp8 + bf16 encode at batch 64 and nothing else (run under rocprofv3 --kernel-trace).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evi_rag_amd import mx, ops  # noqa: E402
from evi_rag_amd.text_encode import TextEncoder  # noqa: E402

FP8_PEAK, BF16_PEAK = 5.0e15, 2.5e15


def _time(fn, dev, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(torch.cuda.current_stream(dev))
    for _ in range(iters):
        fn()
    end.record(torch.cuda.current_stream(dev))
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e-3


def bench_linear(dev, reps=5):
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for K, N in ((1024, 1024), (1024, 4096), (4096, 1024), (768, 3072), (3072, 768)):
        w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
        b = torch.randn(N, device=dev, generator=g)
        wb, bb = w.bfloat16(), b.bfloat16()
        wm = mx.MXWeight(w)
        for M in (2048, 8192, 32768):
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            iters = max(3, int(2e11 / (2 * M * K * N)))
            variants = {"hipblaslt_bf16": lambda: F.linear(x, wb, bb),
                        "mx_linear": lambda: mx.mx_linear(x, wm, b, out_dtype=torch.bfloat16)}
            for fn in variants.values():  # warm: library handles, kernels, caches
                fn()
            torch.cuda.synchronize(dev)
            times = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    times[k].append(_time(fn, dev, iters))
            flop = 2.0 * M * K * N
            row = {"M": M, "K": K, "N": N}
            for k, ts in times.items():
                t = statistics.median(ts)
                row[k] = {"us": t * 1e6, "tflops": flop / t / 1e12}
            row["mx_linear"]["share_of_fp8_peak"] = flop / (row["mx_linear"]["us"] * 1e-6) / FP8_PEAK
            row["hipblaslt_bf16"]["share_of_bf16_peak"] = flop / (row["hipblaslt_bf16"]["us"] * 1e-6) / BF16_PEAK
            row["speedup"] = row["hipblaslt_bf16"]["us"] / row["mx_linear"]["us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


class _LengthTokenizer:
    """Text "i" has lengths[i] random token ids; a batch is padded to its longest text (as bench.py's)."""

    def __init__(self, lengths):
        self.lengths = lengths

    def __call__(self, batch, padding=True, truncation=True, return_tensors="pt"):
        lens = [self.lengths[int(t)] for t in batch]
        L = max(lens)
        g = torch.Generator().manual_seed(int(batch[0]))
        ids = torch.randint(1000, 30000, (len(batch), L), generator=g)
        mask = (torch.arange(L).view(1, L) < torch.tensor(lens).view(-1, 1)).to(torch.int64)
        return {"input_ids": ids * mask, "attention_mask": mask}


def _bert(dev):
    from transformers import BertConfig, BertModel

    torch.manual_seed(0)
    return BertModel(BertConfig(vocab_size=30522, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                intermediate_size=4096, max_position_embeddings=512), add_pooling_layer=False).to(dev).eval()


VARIANTS = {"f32": (None, None), "bf16_autocast": (None, torch.bfloat16), "mxfp8": ("mxfp8", None),
            "mxfp8_bf16_autocast": ("mxfp8", torch.bfloat16)}


def bench_encode(dev, texts=4096, reps=3, batch_sizes=(64, 512), variants=VARIANTS, trace_only=False):
    model = _bert(dev)
    lengths = np.random.default_rng(0).integers(8, 33, texts)
    names = [str(i) for i in range(texts)]
    plain = TextEncoder.from_components(_LengthTokenizer(lengths), model, str(dev), fp16=False)
    mxenc = TextEncoder.from_components(_LengthTokenizer(lengths), copy.deepcopy(model), str(dev), fp16=False, precision="mxfp8")
    encs = {name: (mxenc if prec else plain, ac) for name, (prec, ac) in variants.items()}
    out = {}
    for bs in batch_sizes:
        tables, best = {}, {}
        for name, (enc, ac) in encs.items():  # warm: every (batch, length) shape met twice, so captured and replayed
            enc.autocast = ac
            for _ in range(2):
                tables[name] = enc.encode_to_device(names, bs)
            torch.cuda.synchronize(dev)
            best[name] = float("inf")
        if trace_only:
            return {}
        for _ in range(reps):
            for name, (enc, ac) in encs.items():
                enc.autocast = ac
                t0 = time.perf_counter()
                tables[name] = enc.encode_to_device(names, bs)
                torch.cuda.synchronize(dev)
                best[name] = min(best[name], time.perf_counter() - t0)
        ref = ops.normalize_embeddings(tables["f32"])
        _, i_ref = ops.cosine_topk(ref[:32].contiguous(), ref, 100)
        res = {}
        for name, t in best.items():
            emb = tables[name]
            rel = ((emb - tables["f32"]).norm(dim=1) / tables["f32"].norm(dim=1).clamp(min=1e-30)).max()
            nrm = ops.normalize_embeddings(emb)
            _, idx = ops.cosine_topk(nrm[:32].contiguous(), nrm, 100)
            ov = (idx.unsqueeze(2) == i_ref.unsqueeze(1)).any(dim=2).float().sum(dim=1).div(100).mean()
            res[name] = {"texts_per_s": texts / t, "ms_per_batch": t / (texts / bs) * 1e3, "overlap_at_100_vs_f32": float(ov),
                         "max_rel_row_error_vs_f32": float(rel)}
        res["speedup_mxfp8_bf16_over_bf16"] = best["bf16_autocast"] / best["mxfp8_bf16_autocast"]
        out[f"batch_{bs}"] = res
        print(json.dumps({f"batch_{bs}": res}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-linear", action="store_true")
    ap.add_argument("--skip-encode", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_only:
        bench_encode(dev, batch_sizes=(64,), variants={"mxfp8_bf16_autocast": VARIANTS["mxfp8_bf16_autocast"]}, trace_only=True)
        return
    res = {"device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        if not a.skip_linear:
            res["linear"] = bench_linear(dev)
        if not a.skip_encode:
            res["encode"] = bench_encode(dev)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
