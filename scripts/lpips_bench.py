#!/usr/bin/env python
"""
Times the evaluation metrics on the GPU (synthetic He-scaled weights; the cost does not depend on their values):
  LPIPS on a bench-size batch (256 sequences x 19 predictions = 4864 pairs at 64x64), LPIPS on 576 pairs at 336x336
  (the shipped ExtendedDINOSAUR resolution) and the banded PSNR / SSIM kernel on the same 576 frames at 336x336.
Prints one line per case: ms per call (median of --reps after --warmup) and, for LPIPS, the fraction of the 155 TF/s
fp32-MFMA rate its AlexNet convolutions (both images of every pair) represent.
    python scripts/lpips_bench.py [--reps 5] [--warmup 2]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from textocvp_amd import kernels as K  # noqa: E402

FP32_MFMA_TFLOPS = 155.0


def conv_flop_per_image(H, W):
    flop, h, w = 0, H, W
    for l, (ks, cin, cout) in enumerate(K.LPIPS_LAYERS):
        stride, pad = (4, 2) if l == 0 else (1, ks // 2)
        h, w = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        flop += 2 * h * w * ks * ks * cin * cout
        if l < 2:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return flop


def packed_weights(dev):
    g = torch.Generator().manual_seed(0)
    cw = [torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5 for k, ci, co in K.LPIPS_LAYERS]
    cb = [torch.randn(co, generator=g) * 0.05 for _, _, co in K.LPIPS_LAYERS]
    lin = [torch.rand(co, generator=g) * 0.2 for _, _, co in K.LPIPS_LAYERS]
    return K.pack_lpips_weights(cw, cb, lin, device=dev)


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    packed = packed_weights(dev)
    for n, S in ((4864, 64), (576, 336)):
        g = torch.Generator(device=dev).manual_seed(S)
        x = torch.rand(n, 3, S, S, device=dev, generator=g)
        y = torch.rand(n, 3, S, S, device=dev, generator=g)
        ms = time_ms(lambda: K.lpips(x, y, packed), args.reps, args.warmup)
        tflop = 2 * n * conv_flop_per_image(S, S) / 1e12
        print(f"lpips      {n:5d} pairs {S}x{S}: {ms:9.3f} ms  {tflop:.3f} TFLOP  "
              f"{tflop / (ms * 1e-3) / FP32_MFMA_TFLOPS:.3f} of the fp32-MFMA rate")
        del x, y
    n, S = 576, 336
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, 3, S, S, device=dev, generator=g)
    y = torch.rand(n, 3, S, S, device=dev, generator=g)
    ms = time_ms(lambda: K.psnr_ssim(x, y), args.reps, args.warmup)
    print(f"psnr_ssim  {n:5d} frames {S}x{S} (banded): {ms:9.3f} ms")


if __name__ == "__main__":
    main()
