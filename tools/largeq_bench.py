#!/usr/bin/env python3
"""Many-query top-k: the 32-queries-per-pass scan vs the one-pass GEMM-shaped path, same index, same results.
usage: python tools/largeq_bench.py [rows] [Q] [k] [--index-dtype f32|fp8] [--fp8-mfma 0|1] [--dim D]

--index-dtype f32 (default): the f32 index, all selection precisions, in this process.
--index-dtype fp8: the e4m3 index (quantize_rows_fp8).  The scan and the many-query pass are two steps, each a child
  process of its own under `timeout` (a step that faults, aborts or runs out of time ends the run: nothing more is started
  on the device); each prints one JSON line with the median and the spread of its timed batches."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_index(N, D, dev, g):
    import torch

    from evi_rag_amd import ops

    x = torch.empty((N, D), dtype=torch.float32, device=dev)
    for lo in range(0, N, 1 << 20):
        hi = min(N, lo + (1 << 20))
        x[lo:hi] = ops.normalize_embeddings(torch.randn(hi - lo, D, device=dev, generator=g))
    return x


def main_f32(N, Q, k, D):
    import torch

    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = make_index(N, D, dev, g)
    q = ops.normalize_embeddings(torch.randn(Q, D, device=dev, generator=g))

    def timed(fn, iters=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters, out

    t_scan, (s0, i0) = timed(lambda: ops.cosine_topk(q, x, k))
    t_gemm, (s1, i1) = timed(lambda: ops.cosine_topk_gemm(q, x, k, fallback=False, products=3))
    t_g1, (s2, i2) = timed(lambda: ops.cosine_topk_gemm(q, x, k, fallback=False, products=1))
    shadow = ops.index_shadow_bf16(x)
    t_sh, (s3, i3) = timed(lambda: ops.cosine_topk_gemm(q, x, k, fallback=False, products=1, shadow=shadow))
    same = bool(torch.equal(i0, i1) and torch.equal(s0, s1) and torch.equal(i0, i2) and torch.equal(s0, s2)
                and torch.equal(i0, i3) and torch.equal(s0, s3))
    flops = 2.0 * N * Q * D
    print(f"N={N} Q={Q} k={k} D={D}: scan {t_scan * 1e3:.1f} ms ({Q / t_scan:.0f} q/s, {flops / t_scan / 1e12:.0f} TF/s f32-MFMA), "
          f"gemm {t_gemm * 1e3:.1f} ms ({Q / t_gemm:.0f} q/s, {flops / t_gemm / 1e12:.0f} TF/s algorithmic), "
          f"speedup {t_scan / t_gemm:.2f}x; plain-bf16 selection {t_g1 * 1e3:.1f} ms ({Q / t_g1:.0f} q/s), speedup {t_scan / t_g1:.2f}x; "
          f"with a bf16 shadow index {t_sh * 1e3:.1f} ms ({Q / t_sh:.0f} q/s), speedup {t_scan / t_sh:.2f}x; "
          f"identical results: {same}", flush=True)


def fp8_index(N, D, dev, g):
    """e4m3 codes [N, D] and row scales of normalised Gaussian rows, built 2^20 rows at a time (no f32 copy of the index)."""
    import torch

    from evi_rag_amd import ops

    codes = torch.empty((N, D), dtype=torch.uint8, device=dev)
    scale = torch.empty(N, dtype=torch.float32, device=dev)
    for lo in range(0, N, 1 << 20):
        hi = min(N, lo + (1 << 20))
        c, s = ops.quantize_rows_fp8(ops.normalize_embeddings(torch.randn(hi - lo, D, device=dev, generator=g)))
        codes[lo:hi] = c
        scale[lo:hi] = s
    return codes, scale


def executed_work(step, N, Q, D):
    """(MFMA flops executed, index bytes streamed) per batch.  Both scan variants run two MFMAs per k-step and 16-query block
    over ceil(Q / 32) passes with the query blocks padded to 16; the many-query pass runs two bf16 products over query
    tiles of 256 and reads the index once."""
    if step == "scan":
        passes = -(-Q // 32)
        q_pad = (Q // 32) * 32 + (-(-(Q % 32) // 16)) * 16
        return 2.0 * 2 * N * D * q_pad, float(passes) * N * (D + 4)
    return 2.0 * 2 * N * D * (-(-Q // 256) * 256), float(N) * (D + 4)


def step_fp8(step, N, Q, k, D, native, iters):
    """One step in this process: build the index, warm up, time `iters` batches one by one; one JSON line."""
    import statistics

    import torch

    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    codes, scale = fp8_index(N, D, dev, g)
    q = ops.normalize_embeddings(torch.randn(Q, D, device=dev, generator=g))
    if step == "scan":
        fn = lambda: ops.cosine_topk(q, codes, k, row_scale=scale, method="scan", fp8_mfma=native)
    else:
        fn = lambda: ops.cosine_topk(q, codes, k, row_scale=scale, method="gemm", fp8_mfma=native)
    for _ in range(2):  # the first many-query call also verifies the row norms once (cached on the index)
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(times)
    flops, nbytes = executed_work(step, N, Q, D)
    rec = {"step": step, "N": N, "Q": Q, "k": k, "D": D, "fp8_mfma": int(native), "ms_median": round(med, 3),
           "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "iters": iters,
           "last_method": ops.cosine_topk.last_method,
           "proof_status": ops.cosine_topk_gemm.last_status if step == "gemm" else None,
           "proved_by": ops.cosine_topk_gemm.last_products if step == "gemm" else None,
           "executed_tflops": round(flops / med / 1e9, 1), "index_tb_per_s": round(nbytes / med / 1e9, 3),
           "checksum": [float(out[0].double().sum()), int(out[1].sum())]}
    print(json.dumps(rec), flush=True)


def main_fp8(args):
    """The two steps as children under `timeout`; the first that does not end cleanly ends the run."""
    records = []
    for step in ("scan", "gemm"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), str(args.rows), str(args.Q),
               str(args.k), "--index-dtype", "fp8", "--fp8-mfma", str(args.fp8_mfma), "--dim", str(args.dim), "--iters",
               str(args.iters), "--step", step]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(proc.stdout)
        sys.stdout.flush()
        if proc.returncode != 0:
            print(f"step {step} ended with status {proc.returncode}: stopping", flush=True)
            return proc.returncode if proc.returncode > 0 else 1
        records.append(json.loads(proc.stdout.strip().splitlines()[-1]))
    scan, gemm = records
    print(f"N={args.rows} Q={args.Q} k={args.k} D={args.dim} e4m3 fp8_mfma={args.fp8_mfma}: scan {scan['ms_median']:.2f} ms "
          f"[{scan['ms_min']:.2f}, {scan['ms_max']:.2f}] ({scan['executed_tflops']:.0f} TF/s, {scan['index_tb_per_s']:.2f} TB/s), "
          f"many-query {gemm['ms_median']:.2f} ms [{gemm['ms_min']:.2f}, {gemm['ms_max']:.2f}] ({gemm['executed_tflops']:.0f} TF/s, "
          f"{gemm['index_tb_per_s']:.2f} TB/s), last_method {gemm['last_method']}, proof status {gemm['proof_status']}, "
          f"speedup {scan['ms_median'] / gemm['ms_median']:.2f}x, identical results: {scan['checksum'] == gemm['checksum']}",
          flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rows", nargs="?", type=int, default=1 << 23)
    ap.add_argument("Q", nargs="?", type=int, default=512)
    ap.add_argument("k", nargs="?", type=int, default=500)
    ap.add_argument("--index-dtype", choices=("f32", "fp8"), default="f32")
    ap.add_argument("--fp8-mfma", type=int, choices=(0, 1), default=1)
    ap.add_argument("--dim", type=int, default=None, help="row length (default 768; 1024 for fp8)")
    ap.add_argument("--iters", type=int, default=7, help="timed batches per step (fp8)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each fp8 step may take")
    ap.add_argument("--step", choices=("scan", "gemm"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.dim is None:
        args.dim = 1024 if args.index_dtype == "fp8" else 768
    if args.index_dtype == "f32":
        return main_f32(args.rows, args.Q, args.k, args.dim)
    if args.step:
        return step_fp8(args.step, args.rows, args.Q, args.k, args.dim, bool(args.fp8_mfma), args.iters)
    return main_fp8(args)


if __name__ == "__main__":
    sys.exit(main())
