"""
Decoder loss + backward of the SAVi ``up2`` variant (GenericDecoderLoss, training step) on one device, on the 2040 slot
images (68 frames x 30 slots) of scripts/savi_variants_timing.py: milliseconds of the forward decode and of the loss +
backward (ratio), and the device time of every convk forward and convk_dgrad launch of one loss + backward in TFLOP/s and
as a fraction of the bf16 dense matrix peak (2516.6 TFLOP/s).  FLOPs are those the kernels execute (dgrad under up2: a
stride-2 (k + 1)^2-tap correlation per source pixel), a split product counted once.
    python scripts/savi_train_timing.py [--iters 10] [--out profiles/savi_train_timing.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/savi_train_timing.py --profile   # one loss + backward
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from textocvp_amd import kernels as K  # noqa: E402
from textocvp_amd import synth  # noqa: E402
from textocvp_amd.train.decoder_generic import GenericDecoderLoss  # noqa: E402
from savi_variants_timing import FRAMES, SLOTS, model  # noqa: E402

PEAK_TFLOPS = 2516.6


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one loss + backward, nothing else")
    args = ap.parse_args()
    savi = model("up2")
    slots = synth.synth_tensor("timing.slots", (FRAMES, SLOTS, 128), "normal").cuda()
    targets = synth.synth_tensor("timing.targets", (FRAMES, 3, 64, 64), "unit").cuda()
    loss = GenericDecoderLoss(savi)
    gs = 2.0 / targets.numel()
    if args.profile:
        for _ in range(2):
            loss.loss_and_slot_grad(slots, targets, gs)
            torch.cuda.synchronize()
        return
    with torch.no_grad():
        fwd = timed(lambda: savi.decode(slots), args.iters)
    bwd = timed(lambda: loss.loss_and_slot_grad(slots, targets, gs), args.iters)
    res = {"slot_images": FRAMES * SLOTS, "device": torch.cuda.get_device_name(0), "decode_ms": fwd,
           "loss_and_backward_ms": bwd, "backward_over_decode": bwd / fwd, "launches": {}}
    K.TIMER = K.LaunchTimer(only=("convk",))
    try:
        loss.loss_and_slot_grad(slots, targets, gs)
        torch.cuda.synchronize()
        for name, s in sorted(K.TIMER.summary().items()):
            ms = s["total_ms"] / s["launches"]
            tf = s["units"] / s["launches"] / (ms * 1e-3) / 1e12
            res["launches"][name] = {"ms": ms, "tflops": tf, "of_bf16_peak": tf / PEAK_TFLOPS}
    finally:
        K.TIMER = None
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
